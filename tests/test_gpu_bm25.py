"""BM25 ranking on the device (sme_query_topk_bm25*): every output is held bit for bit
to the restatement of bm25_ref.py over the index's own reduce-order CSR (Index.csr()):
docno arrays equal, score.view(int64) equal, which includes the order, the cut and the
pads.  Crafted indexes loaded from hand-written record streams put posting lists on the
scorer's window edges (taken from bm25_stats()["window"]), reach the window skip and
run the candidate list's cut over and over; a built index with negative docnos holds
the document lengths to the kept term streams, and its reopened, merged and deleted-from
forms to the restatement over their own CSR."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import bm25_ref as R
import common
import load_streams as S
import posfile_ref

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
PARAMS = [(1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (0.9, 1.0)]
KS = (1, 3, 10, 64, 65, 1024)
SPLITS = (0, 1, 3, 10 ** 6)
A, BIG, C_, EDGE, F63, F64, F65, HI, NONE, ONE, R_ = range(11)  # ids in key order (names below)
NAMES = [b"ta", b"tbig", b"tc", b"tedge", b"tf63", b"tf64", b"tf65", b"thi", b"tnone", b"tone", b"tr"]
assert NAMES == sorted(NAMES)


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:8]
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), np.argwhere(got[1] != want[1])[:8]


def _load(sme, lists, n_docs):
    """An index from {name: [(docno, tf)]}, names in key order, docnos 1..n_docs."""
    recs = [S.record(name, sorted(posts, key=lambda p: (-p[1], p[0]))) for name, posts in lists]
    ix = sme.Context(1, 1, 1).load_records([b"".join(recs), S.counter(S.counter_posts(list(range(1, n_docs + 1))))])
    assert ix.V == len(lists) and ix.N == n_docs
    return ix


def _lists_s(n, W):
    last = n
    return [
        (NAMES[A], [(d, 1 + d % 3) for d in range(1, n + 1)]),
        (NAMES[BIG], [(d, 1000) for d in (100, n // 2 + 500, last)]),
        (NAMES[C_], [(d, 1 + 7 * d % 5) for d in range(2, n + 1, 2)]),
        (NAMES[EDGE], [(1 + o, 5) for o in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)]),
        (NAMES[F63], [(d, 2) for d in range(1, 64)]),
        (NAMES[F64], [(d, 2) for d in range(1, 65)]),
        (NAMES[F65], [(d, 2) for d in range(1, 66)]),
        (NAMES[HI], [(d, 1 + d % 4) for d in range(last - 499, last + 1)]),
        (NAMES[NONE], []),
        (NAMES[ONE], [(4321, 7)]),
        (NAMES[R_], [(d, 3) for d in (5, 6, 7, last - 1)]),
    ]


@pytest.fixture(scope="module")
def crafted(sme):
    """(index S, its restatement, docs, window)."""
    n = 9000
    ix = _load(sme, _lists_s(n, 1024), n)
    W = ix.bm25_stats()["window"]
    if n < 3 * W or W != 1024:
        n = max(n, 3 * W + 1000)
        ix = _load(sme, _lists_s(n, W), n)
    ref = R.Ref.from_csr(ix.csr())
    return ix, ref, n, W


QUERIES = [[t] for t in range(11)] + [
    [A, C_], [R_, A, C_], [C_, R_], [HI, EDGE, BIG], [F63, F64, F65], [ONE, NONE], [EDGE, ONE, A],
    [A, A, C_], [C_, C_], [R_, R_, R_, A],            # duplicates count twice
    [-1, A, -1, C_], [EDGE, -1], [-1, -1, ONE],          # -1 mixed in
    [], [-1], [NONE], [NONE, -1, NONE],
    [BIG, HI], [F65, HI],
    ([R_, -1, F63, NONE, EDGE] * 205)[:1020] + [A, C_, BIG, HI],  # 1024 slots
]


def _run(ix, ref, queries, k, k1, b):
    ids, off = R.batch(queries)
    _same(ix.query_bm25(ids, off, k, k1, b), ref.run(ids, off, k, k1, b))


def test_statistics(crafted):
    ix, ref, n, W = crafted
    st = ix.bm25_stats()
    assert (st["docs"], st["total_len"], st["max_len"]) == (ref.D, ref.L, int(ref.dl.max())) and ref.D == n
    dmin, dl = ix.doc_lengths()
    assert dmin == ref.dmin == 1 and dl.dtype == np.int32 and np.array_equal(dl, ref.dl)
    assert ix.prepare_bm25() >= 0.0  # built already: nothing happens


def test_by_hand(crafted):
    """Results written out here, so the restatement is not the only witness."""
    ix, ref, n, W = crafted
    dn, sc = ix.query_bm25([ONE, NONE, -1, R_, R_], [0, 1, 2, 3, 5], 5, 0.0, 0.75)
    assert dn.tolist() == [[4321, -1, -1, -1, -1], [-1] * 5, [-1] * 5, [5, 6, 7, n - 1, -1]]
    idf_r = math.log(1.0 + (float(n - 4) + 0.5) / (4.0 + 0.5))
    assert sc[3].tolist() == [idf_r + idf_r] * 4 + [0.0]  # k1 = 0: every posting weighs its idf
    assert sc[0, 0] == math.log(1.0 + (float(n - 1) + 0.5) / (1.0 + 0.5)) and not sc[1].any() and not sc[2].any()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("k1,b", PARAMS)
def test_crafted(crafted, k1, b, split):
    ix, ref, n, W = crafted
    ix.ctx.set_option("bm25_split", split)
    try:
        for k in KS:
            _run(ix, ref, QUERIES, k, k1, b)
    finally:
        ix.ctx.set_option("bm25_split", 0)


def test_each_query_alone(crafted):
    ix, ref, n, W = crafted
    for q in QUERIES:
        _run(ix, ref, [q], 10, 1.2, 0.75)
    dn, sc = ix.query_bm25(np.zeros(0, np.int32), np.zeros(1, np.int64), 4)  # no query at all
    assert dn.shape == (0, 4) and sc.shape == (0, 4)


def test_device_entry(sme, crafted):
    ix, ref, n, W = crafted
    L = sme.lib()
    ids, off = R.batch(QUERIES[:24])
    bad = ids.copy()
    bad[bad == NONE] = ix.V + 5  # the device entry skips an id outside [-1, V) like -1
    nq, k = len(off) - 1, 7
    ptrs = []
    try:
        for nbytes in (bad.nbytes, off.nbytes, 4 * nq * k, 8 * nq * k):
            p = C.c_void_p()
            assert L.sme_device_alloc(0, max(nbytes, 16), C.byref(p)) == 0
            ptrs.append(p)
        sme.memcpy(ptrs[0].value, bad.ctypes.data, bad.nbytes)
        sme.memcpy(ptrs[1].value, off.ctypes.data, off.nbytes)
        ix.query_bm25_device(ptrs[0].value, ptrs[1].value, nq, k, ptrs[2].value, ptrs[3].value, 0.9, 1.0)
        dn, sc = np.zeros((nq, k), np.int32), np.zeros((nq, k), np.float64)
        sme.memcpy(dn.ctypes.data, ptrs[2].value, dn.nbytes)
        sme.memcpy(sc.ctypes.data, ptrs[3].value, sc.nbytes)
        _same((dn, sc), ref.run(ids, off, k, 0.9, 1.0))
    finally:
        for p in ptrs:
            L.sme_device_free(p)


def _raises(sme, call, code, *words):
    with pytest.raises(sme.SmeError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_limits_and_arguments(sme, crafted):
    ix, ref, n, W = crafted
    ids, off = R.batch([[A], [F63] * 1025, [C_]])
    _raises(sme, lambda: ix.query_bm25(ids, off, 3), SME_ELIMIT, "query 1")
    _run(ix, ref, [[A], [F63] * 1024, [C_]], 3, 1.2, 0.75)  # the limit itself, and the next valid call
    _raises(sme, lambda: ix.query_bm25([A], [0, 1], 1025), SME_ELIMIT, "1024")
    _run(ix, ref, [[A]], 1024, 1.2, 0.75)
    for k1, b in ((float("nan"), 0.75), (-0.5, 0.75), (float("inf"), 0.75), (1.2, 1.5), (1.2, -0.1), (1.2, float("nan"))):
        _raises(sme, lambda: ix.query_bm25([A], [0, 1], 3, k1, b), SME_EINVAL, "k1")
    _raises(sme, lambda: ix.query_bm25([A, ix.V], [0, 1, 2], 3), SME_EINVAL, "query 1")
    _raises(sme, lambda: ix.query_bm25([A, -2], [0, 2], 3), SME_EINVAL, "query 0")
    _raises(sme, lambda: ix.query_bm25([A, C_], [0, 2, 1], 3), SME_EINVAL)
    _raises(sme, lambda: ix.query_bm25([A], [0, 1], 0), SME_EINVAL)
    _raises(sme, lambda: ix.ctx.set_option("bm25_split", -1), SME_EINVAL)
    _run(ix, ref, QUERIES[:14], 3, 1.2, 0.75)


def test_skip_path_is_reached(crafted):
    """[R, A, C], k = 3, one workgroup: after the first window the bar is an R document's
    score, and no window without an R document can reach it -- checked here with the
    restatement's arithmetic, for windows of 1024, 2048 and 4096 documents."""
    ix, ref, n, W = crafted
    k1, b = 1.2, 0.75
    dn, sc = ref.scores([R_, A, C_], k1, b)
    bar = np.sort(sc[np.isin(dn, (5, 6, 7))])[0]  # the third best once the first window is seen
    assert 8.0 < bar < 9.0  # (about 8.38: idf_R is 7.6, and documents 5..7 are three times the average length)
    for w in (1024, 2048, 4096):
        for base in range(1, n + 1, w):
            docs = np.arange(base, min(base + w, n + 1))
            if np.isin((5, 6, 7, n - 1), docs).any():
                continue
            mindl = int(min(ref.doc_length(int(d)) for d in docs))
            bound = 0.0
            for t, maxtf in ((A, 3), (C_, 5)):
                bound += R.bound_term(ref.idf[t], maxtf, k1, b, mindl, ref.avgdl)
            assert bound < bar
    ix.ctx.set_option("bm25_split", 1)
    try:
        _run(ix, ref, [[R_, A, C_]], 3, k1, b)
        st = ix.query_bm25_stats()
        total = sum(int(ref.df[t]) for t in (R_, A, C_))
        windows = (n + W - 1) // W
        assert st["windows"] == windows and 1 <= st["skipped"] <= windows - 2
        assert 0 < st["postings"] < total
        _run(ix, ref, [[R_, A, C_]], 5, k1, b)  # the bar is an A + C score here: only equality is asked
        assert ix.query_bm25_stats()["windows"] == windows
    finally:
        ix.ctx.set_option("bm25_split", 0)


@pytest.fixture(scope="module")
def crafted_m(sme):
    n = 9000
    lists = [(b"ta", [(d, 1) for d in range(1, n + 1)]), (b"tz", [(d, 1 + (n - d) // 16) for d in range(1, n + 1)])]
    ix = _load(sme, lists, n)
    return ix, R.Ref.from_csr(ix.csr()), n


@pytest.mark.parametrize("split", [0, 1])
def test_every_document_enters_the_list(crafted_m, split):
    """Index M: [A]'s scores never fall as docnos rise (563 values in runs of 16 ties), so
    every document enters the candidate list and the cut runs again and again; [Z]'s
    never rise."""
    ix, ref, n = crafted_m
    dn, sc = ref.scores([0], 1.2, 0.75)
    assert np.all(np.diff(sc) >= 0) and len(set(sc.tolist())) == 563
    assert all(len(set(sc[i:i + 16].tolist())) == 1 for i in range(8, n - 16, 16))
    dn, sz = ref.scores([1], 1.2, 0.75)
    assert np.all(np.diff(sz) <= 0)
    ix.ctx.set_option("bm25_split", split)
    try:
        for k in (1, 10, 1024):
            _run(ix, ref, [[0], [1], [0, 1]], k, 1.2, 0.75)
    finally:
        ix.ctx.set_option("bm25_split", 0)


# ---- a built index: negative docnos, duplicates, docno 0 ----------------------------------------
@functools.lru_cache(maxsize=None)
def _fuzz():
    corpus, mapping = common.fuzz_corpus(8, 120, extra_docids=40)
    return corpus, mapping


def _ctx(sme, mapping, R_parts=3):
    ctx = sme.Context(1, R_parts, 1)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(mapping))
    ctx.set_option("positions", 1)
    return ctx


def _lengths(ix):
    """{docno: dl} of the documents with postings, from the device's table."""
    dmin, dl = ix.doc_lengths()
    return {dmin + int(i): int(dl[i]) for i in np.nonzero(dl)[0]}


def _ref_lengths(ref):
    return {ref.dmin + int(i): int(ref.dl[i]) for i in np.nonzero(ref.dl)[0]}


def _random_queries(ref, seed, n=60):
    rng = random.Random(seed)
    terms = [t for t in range(ref.V)]
    by_df = sorted(terms, key=lambda t: -int(ref.df[t]))
    out = []
    for _ in range(n):
        pool = by_df[:20] if rng.random() < 0.5 else terms
        out.append([rng.choice(pool) for _ in range(rng.randint(1, 8))])
    return out


@pytest.fixture(scope="module")
def built(sme):
    corpus, mapping = _fuzz()
    ix = _ctx(sme, mapping).build(corpus)
    return ix, R.Ref.from_csr(ix.csr())


def test_built_doc_lengths_equal_stream_lengths(built):
    """An independent witness of dl: the kept term streams hold every index term of a
    record, DOCNO tokens included."""
    ix, ref = built
    _, recs = posfile_ref.decode(ix.positions_file())
    want = {}
    for d, s in recs:
        want[d] = want.get(d, 0) + len(s)
    assert min(want) < 0 and 0 in want  # unmapped docids and records without a DOCNO
    got = _lengths(ix)
    assert got == {d: v for d, v in want.items() if v} == _ref_lengths(ref)
    st = ix.bm25_stats()
    assert (st["docs"], st["total_len"], st["max_len"]) == (len(got), sum(got.values()), max(got.values()))
    assert (ref.D, ref.L) == (st["docs"], st["total_len"])


@pytest.mark.parametrize("k1,b", PARAMS)
def test_built_queries(built, k1, b):
    ix, ref = built
    for k in (1, 10, 200):
        _run(ix, ref, _random_queries(ref, 3), k, k1, b)


def test_reopened_from_parts(sme, built):
    ix, ref = built
    _, mapping = _fuzz()
    again = _ctx(sme, mapping).load_records([ix.partition_records(p) for p in range(3)])
    assert _lengths(again) == _lengths(ix) and again.bm25_stats() == ix.bm25_stats()
    ids, off = R.batch(_random_queries(ref, 4))
    _same(again.query_bm25(ids, off, 10), ix.query_bm25(ids, off, 10))
    _same(again.query_bm25(ids, off, 10), ref.run(ids, off, 10))


def test_merged_and_deleted(sme, built):
    ix, whole = built
    corpus, mapping = _fuzz()
    docs = corpus.split(b"</DOC>\n")
    half = len(docs) // 2
    ctx = _ctx(sme, mapping)
    parts = [ctx.build(b"</DOC>\n".join(docs[:half]) + b"</DOC>\n"), ctx.build(b"</DOC>\n".join(docs[half:]))]
    merged = ctx.merge(parts)
    ref = R.Ref.from_csr(merged.csr())
    assert _lengths(merged) == _ref_lengths(ref) and merged.bm25_stats()["docs"] == ref.D
    _run(merged, ref, _random_queries(ref, 5), 10, 1.2, 0.75)
    gone = random.Random(6).sample(sorted(_ref_lengths(whole)), 10)
    less = ix.delete_docnos(gone)
    lref = R.Ref.from_csr(less.csr())
    assert lref.D == whole.D - 10 and all(lref.doc_length(d) == 0 for d in gone)
    assert _lengths(less) == _ref_lengths(lref) == {d: v for d, v in _ref_lengths(whole).items() if d not in gone}
    _run(less, lref, _random_queries(lref, 7), 10, 0.9, 1.0)


def test_facade_and_topk_untouched(sme, built):
    ix, ref = built
    fwd = sme.IntDocVectorsForwardIndex(ix)
    words = [ix.term(t) for t in sorted(range(ref.V), key=lambda t: -int(ref.df[t]))[:3]]
    fwd.getValue(words + ["nosuchwordatall"])
    ids = ix.lookup(words).tolist()
    assert all(t >= 0 for t in ids)
    want = [int(d) for d in ref.topk(ids, 10)[0] if d >= 0]
    assert fwd.rank_bm25() == want and fwd.rank_bm25(3, 0.9, 1.0) == [int(d) for d in ref.topk(ids, 3, 0.9, 1.0)[0] if d >= 0]
    fwd.getValue(["nosuchwordatall"])
    assert fwd.rank_bm25() == []
    # the TF-IDF scorer's bytes are the same before and after a BM25 call
    qi, qo = R.batch(_random_queries(ref, 9, 20))
    before = ix.query_topk(qi, qo, 10)
    ix.query_bm25(qi, qo, 10)
    after = ix.query_topk(qi, qo, 10)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


def test_no_query_side(sme):
    """A chargram output has no postings by document: SME_EINVAL, as the query entries refuse it."""
    grams = sme.Context(2, 2).build_chargram(b"<DOC>\n<DOCNO> X-1 </DOCNO>\n<TEXT>\nalpha beta\n</TEXT>\n</DOC>\n")
    ms = C.c_float()
    assert sme.lib().sme_index_prepare_bm25(grams._h, None, C.byref(ms)) == SME_EINVAL
    vals = [C.c_uint64() for _ in range(4)]
    assert sme.lib().sme_index_bm25_stats(grams._h, *[C.byref(v) for v in vals]) == SME_EINVAL
