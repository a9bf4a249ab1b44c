"""Scoring given documents on the device (sme_query_rescore*): offsets, docnos and hits
are held exactly, score.view(int64) bit for bit, to the restatement of rescore_ref.py
(pinned by test_rescore_host.py) -- both models, both orders, the cut, min_hits and
every value of "rescore_path".  A crafted index loaded from hand-written record
streams, sized from rescore_stats()["tile"], puts posting lists and candidate lists
on the scorer's tile edges.  Three witnesses that are not the restatement: all docnos
rescored are sme_query_topk_bm25's and sme_query_topk's rows, and a Boolean result
rescored under TF-IDF over its required slots reproduces the Boolean scores."""
import contextlib
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import bm25_ref as R
import common
import load_streams as S
import rescore_ref as RR
import test_gpu_structq as TQ  # (its crafted corpus and helpers; nothing of them is changed)

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
PARAMS = [(1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (0.9, 1.0)]  # test_gpu_bm25's
MODELS = [("tfidf", 1.2, 0.75)] + [("bm25", k1, b) for k1, b in PARAMS]
ORDERS, MS, MIN_HITS, PATHS = (0, 1), (0, 1, 10), (0, 1, 2), (0, 1, 2)
A, BIG, C_, EDGE, FULL, GAP, HI, NONE, ONE, POST, PRE, R_, SPAN = range(13)  # ids in key order (names below)
NAMES = [b"ta", b"tbig", b"tc", b"tedge", b"tfull", b"tgap", b"thi", b"tnone", b"tone", b"tpost", b"tpre", b"tr",
         b"tspan"]
assert NAMES == sorted(NAMES)
LO, HI32 = -2 ** 31, 2 ** 31 - 1


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert got[3].dtype == np.float64
    assert np.array_equal(got[0], want[0]), np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:8]
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:8]
    assert np.array_equal(got[2], want[2]), np.nonzero(got[2] != want[2])[0][:8]
    assert np.array_equal(got[3].view(np.int64), want[3].view(np.int64)), np.nonzero(got[3] != want[3])[0][:8]


def _lists(n, T):
    """Docnos 1 .. n, n = 3 T + 500.  With all docnos as candidates the tiles are
    [1, T], [T + 1, 2 T], [2 T + 1, 3 T], [3 T + 1, n]."""
    return [
        (NAMES[A], [(d, 1 + d % 3) for d in range(1, n + 1)]),
        (NAMES[BIG], [(d, 1000) for d in (100, n // 2 + 500, n)]),
        (NAMES[C_], [(d, 1 + 7 * d % 5) for d in range(2, n + 1, 2)]),
        # first and last postings exactly at tiles' last and first candidates
        (NAMES[EDGE], [(d, 5) for d in (T, T + 1, 2 * T, 2 * T + 1, 3 * T, 3 * T + 1)]),
        (NAMES[FULL], [(d, 2) for d in range(T + 1, 2 * T + 1)]),  # one whole tile, edge to edge
        (NAMES[GAP], [(d, 3) for d in range(70, 101)]),  # wholly between the candidates 65 and 129 of SPARSE
        (NAMES[HI], [(d, 1 + d % 4) for d in range(n - 499, n + 1)]),
        (NAMES[NONE], []),
        (NAMES[ONE], [(T + 500, 7)]),
        (NAMES[POST], [(d, 2) for d in range(2 * T + 1, 2 * T + 7)]),  # starts just after the tile [T + 1, 2 T]
        (NAMES[PRE], [(d, 4) for d in range(T - 5, T + 1)]),  # ends just before it
        (NAMES[R_], [(d, 3) for d in (5, 6, 7, n - 1)]),
        (NAMES[SPAN], [(d, 1 + d % 2) for d in range(T - 9, 2 * T + 11)]),  # three tiles
    ]


def _load(sme, n, T):
    recs = [S.record(name, sorted(posts, key=lambda p: (-p[1], p[0]))) for name, posts in _lists(n, T)]
    ix = sme.Context(1, 1, 1).load_records([b"".join(recs), S.counter(S.counter_posts(list(range(1, n + 1))))])
    assert ix.V == len(NAMES) and ix.N == n
    return ix


@pytest.fixture(scope="module")
def crafted(sme):
    """(index, its restatement, docs, tile)."""
    T = 1024
    ix = _load(sme, 3 * T + 500, T)
    if ix.rescore_stats()["tile"] != T:
        T = ix.rescore_stats()["tile"]
        ix = _load(sme, 3 * T + 500, T)
    n = 3 * T + 500
    ref = RR.Ref(R.Ref.from_csr(ix.csr()), ix.weights())
    assert ref.bm.dmin == 1 and ref.bm.span == n
    return ix, ref, n, T


def _cands(n, T):
    rng = random.Random(11)
    return {
        "all": list(range(1, n + 1)),
        "even": list(range(2, n + 1, 2)),
        "third": list(range(1, n + 1, 3)),
        "T-1": list(range(2, T + 1)),
        "T": list(range(T + 1, 2 * T + 1)),  # one tile: PRE ends just before it, POST starts just after
        "T+1": list(range(T, 2 * T + 1)),
        "2T+1": list(range(T - 3, 3 * T - 2)),
        "sparse": list(range(1, n + 1, 64)),  # gaps wider than GAP, EDGE's, PRE and POST
        "outside": [LO, -5, 0, 3, 5, T, T + 500, n, n + 1, n + 100, HI32],  # below dmin and above dmax
        "below": [LO, -7, 0],
        "random": sorted(rng.sample(range(1, n + 1), T + T // 2)),
        "none": [],
        "one": [T + 500],
    }


SLOTS = [[t] for t in range(13)] + [
    [A, C_], [R_, A, C_], [HI, EDGE, BIG], [PRE, FULL, POST], [SPAN, GAP, ONE], [EDGE, SPAN, FULL],
    [A, A, C_], [R_, R_, R_, A], [FULL, SPAN, FULL],  # duplicates count twice
    [-1, A, -1, C_], [EDGE, -1], [-1, -1, ONE],  # -1 mixed in
    [-1], [-1, -1], [], [NONE], [NONE, -1, NONE],
    ([R_, -1, SPAN, NONE, EDGE] * 205)[:1020] + [A, C_, BIG, HI],  # 1024 slots
]


@functools.lru_cache(maxsize=None)
def _queries(n, T):
    cl = _cands(n, T)
    assert [len(cl[k]) for k in ("T-1", "T", "T+1", "2T+1")] == [T - 1, T, T + 1, 2 * T + 1]
    return [(s, c) for s in SLOTS for c in cl.values()]


def _stats_of(ref, queries, model, k1, b, min_hits):
    found = matches = 0
    for s, c in queries:
        hits = ref.score(s, c, model, k1, b)[0]
        found += int(hits.sum())
        matches += int((hits >= min_hits).sum())
    return {"candidates": sum(len(c) for _, c in queries), "found": found, "matches": matches}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("model,k1,b", MODELS)
def test_crafted(crafted, model, k1, b, path):
    ix, ref, n, T = crafted
    queries = _queries(n, T)
    arrays = RR.batch(queries)
    ix.ctx.set_option("rescore_path", path)
    try:
        for order in ORDERS:
            for m in MS:
                for min_hits in MIN_HITS:
                    got = ix.rescore(*arrays, model=model, order=order, m=m, min_hits=min_hits, k1=k1, b=b)
                    _same(got, ref.run(queries, model, order, m, min_hits, k1, b))
        st = ix.rescore_stats()
        assert st.pop("tile") == T and st == _stats_of(ref, queries, model, k1, b, MIN_HITS[-1])
    finally:
        ix.ctx.set_option("rescore_path", 0)


def test_each_query_alone_and_none(sme, crafted):
    ix, ref, n, T = crafted
    for q in _queries(n, T)[::7]:
        _same(ix.rescore(*RR.batch([q]), model="bm25", order=1, m=5, min_hits=1), ref.run([q], "bm25", 1, 5, 1))
    got = ix.rescore(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64))
    assert got[0].tolist() == [0] and all(x.size == 0 for x in got[1:])  # nq == 0
    assert ix.rescore_stats() == {"candidates": 0, "found": 0, "matches": 0, "tile": T}
    outs = [C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()]
    assert sme.lib().sme_query_rescore(ix._h, None, None, None, None, 0, 1, 1.2, 0.75, 0, 1, 0,
                                       *[C.byref(o) for o in outs]) == 0  # no array at all
    assert outs[0][0] == 0


def test_by_hand(crafted):
    """Results written out here, so the restatement is not the only witness."""
    ix, ref, n, T = crafted
    off, dn, hits, sc = ix.rescore([R_, R_, ONE, -1], [0, 4], [4, 5, 7, T + 500, n, n + 9], [0, 6], model="bm25",
                                   order=1, k1=0.0)
    idf_r = math.log(1.0 + (float(n - 4) + 0.5) / (4.0 + 0.5))
    idf_one = math.log(1.0 + (float(n - 1) + 0.5) / (1.0 + 0.5))
    assert off.tolist() == [0, 6] and dn.tolist() == [5, 7, T + 500, 4, n, n + 9]  # k1 = 0: a posting weighs its idf
    assert hits.tolist() == [2, 2, 1, 0, 0, 0] and sc.tolist() == [idf_r + idf_r] * 2 + [idf_one, 0.0, 0.0, 0.0]
    off, dn, hits, sc = ix.rescore([R_, ONE], [0, 2], [4, 5, 7, T + 500], [0, 4], model="tfidf", order=0, min_hits=1, m=2)
    assert dn.tolist() == [5, 7] and hits.tolist() == [1, 1] and sc[0] == sc[1] > 0.0


# ---- the three witnesses ---------------------------------------------------------------------
WITNESS = [[C_, R_], [HI, EDGE, BIG], [R_], [SPAN, GAP, ONE], [FULL, FULL, PRE], [-1, POST, C_], [EDGE], [NONE], []]


@pytest.mark.parametrize("k", (1, 10, 1024))
def test_witness_bm25_topk(crafted, k):
    ix, ref, n, T = crafted
    queries = WITNESS + [[A, C_]]
    ids, qoff = R.batch(queries)
    dn, sc = ix.query_bm25(ids, qoff, k, 0.9, 1.0)
    every = np.arange(1, n + 1, dtype=np.int32)
    got = ix.rescore(ids, qoff, np.tile(every, len(queries)), np.arange(len(queries) + 1, dtype=np.int64) * n,
                     model="bm25", order=1, m=k, min_hits=1, k1=0.9, b=1.0)
    for q in range(len(queries)):
        row = dn[q] >= 0
        a, e = got[0][q], got[0][q + 1]
        assert np.array_equal(got[1][a:e], dn[q][row]) and e - a == row.sum()
        assert np.array_equal(got[3][a:e].view(np.int64), sc[q][row].view(np.int64))


@pytest.mark.parametrize("k", (1, 10, 1024))
def test_witness_tfidf_topk(crafted, k):
    """sme_query_topk under SME_TIE_DOCNO (the context's default)."""
    ix, ref, n, T = crafted
    ids, qoff = R.batch(WITNESS)
    dn, sc = ix.query_topk(ids, qoff, k)
    every = np.arange(1, n + 1, dtype=np.int32)
    got = ix.rescore(ids, qoff, np.tile(every, len(WITNESS)), np.arange(len(WITNESS) + 1, dtype=np.int64) * n,
                     model="tfidf", order=1, m=k, min_hits=1)
    for q in range(len(WITNESS)):
        row = dn[q] >= 0
        a, e = got[0][q], got[0][q + 1]
        assert np.array_equal(got[1][a:e], dn[q][row]) and e - a == row.sum()
        assert np.array_equal(got[3][a:e].view(np.int64), sc[q][row].view(np.int64))


BOOLEAN = [
    [([A], False), ([C_], False)],
    [([R_, BIG], False), ([C_, SPAN], False), ([HI], True)],
    [([SPAN], False), ([FULL], False), ([EDGE, PRE, POST], False)],
    [([C_, C_], False), ([A], False), ([GAP], True)],
    [([ONE], False)], [([NONE], False)], [([R_], False), ([-1], True)], [],
]


def _required(groups):
    return [t for ids, excluded in groups if not excluded for t in ids]


def test_witness_boolean_scores(crafted):
    ix, ref, n, T = crafted
    boff, bdn, bsc = ix.query_boolean(BOOLEAN, order=0, m=0)
    assert boff[-1] > 2 * T  # more than one tile
    ids, qoff = R.batch([_required(g) for g in BOOLEAN])
    off, dn, hits, sc = ix.rescore(ids, qoff, bdn, boff, model="tfidf", order=0, m=0, min_hits=0)
    assert np.array_equal(off, boff) and np.array_equal(dn, bdn)
    assert np.array_equal(sc.view(np.int64), bsc.view(np.int64)) and hits.min() >= 1


# ---- the device entry, and the other features' buffers ------------------------------------------
@contextlib.contextmanager
def _on_device(sme, *arrays):
    L = sme.lib()
    ptrs = []
    try:
        for a in arrays:
            p = C.c_void_p()
            assert L.sme_device_alloc(0, max(a.nbytes, 16), C.byref(p)) == 0
            ptrs.append(p)
            if a.nbytes:
                sme.memcpy(p.value, a.ctypes.data, a.nbytes)
        yield [p.value for p in ptrs]
    finally:
        for p in ptrs:
            L.sme_device_free(p)


def _fetch(sme, ptr, count, dt):
    a = np.zeros(count, dt)
    if count:
        sme.memcpy(a.ctypes.data, ptr, a.nbytes)
    return a


def _fetch_result(sme, r, nq):
    return (_fetch(sme, r[0], nq + 1, np.int64), _fetch(sme, r[1], r[4], np.int32), _fetch(sme, r[2], r[4], np.int32),
            _fetch(sme, r[3], r[4], np.float64))


def test_device_entry_crafted(sme, crafted):
    ix, ref, n, T = crafted
    queries = _queries(n, T)[::3]
    ids, qoff, docs, doff = RR.batch(queries)
    with _on_device(sme, docs, doff) as (d_docs, d_doff):
        for order, m, min_hits in ((1, 10, 1), (0, 0, 0), (0, 3, 2)):
            r = ix.rescore_device(ids, qoff, d_docs, d_doff, model="bm25", order=order, m=m, min_hits=min_hits, k1=2.0,
                                  b=0.0)
            got = _fetch_result(sme, r, len(queries))
            _same(got, ref.run(queries, "bm25", order, m, min_hits, 2.0, 0.0))
            _same(got, ix.rescore(ids, qoff, docs, doff, model="bm25", order=order, m=m, min_hits=min_hits, k1=2.0,
                                  b=0.0))


def test_boolean_device_result_goes_in_unchanged(sme, crafted):
    ix, ref, n, T = crafted
    boff, bdn, _ = ix.query_boolean(BOOLEAN, order=0, m=0)
    ids, qoff = R.batch([_required(g) for g in BOOLEAN])
    host = ix.rescore(ids, qoff, bdn, boff, model="bm25", order=1, m=7, min_hits=0)
    d_off, d_dn, d_sc, total = ix.query_boolean_device(BOOLEAN, order=0, m=0)
    assert total == boff[-1]
    r = ix.rescore_device(ids, qoff, d_dn, d_off, model="bm25", order=1, m=7, min_hits=0)
    _same(_fetch_result(sme, r, len(BOOLEAN)), host)
    _same(host, ref.run([(_required(g), bdn[boff[i]:boff[i + 1]]) for i, g in enumerate(BOOLEAN)], "bm25", 1, 7, 0))


def test_other_features_results_stay(sme):
    corpus, mapping, st = TQ._craft()
    ix = TQ._ctx(sme, mapping, 1, 0).build(corpus)
    kilo, lima, mike, zulu = TQ._words(ix, "kilo", "lima", "mike", "zulu")
    bq = [[([kilo], False), ([mike], False)]]
    b = ix.query_boolean(bq, 1, 5)
    p = ix.query_phrase([[kilo, lima]], 0, 6)
    d_b = ix.query_boolean_device(bq, 1, 5)
    d_p = ix.query_phrase_device([[kilo, lima]], 0, 6)
    ids, qoff = R.batch([[kilo, mike], [zulu]])
    bm = ix.query_bm25(ids, qoff, 8)
    bm_stats = ix.query_bm25_stats()
    pall = ix.query_phrase([[kilo, lima]], 0, 0)
    d_all = ix.query_phrase_device([[kilo, lima]], 0, 0)  # (the phrase result the rescore reads)
    r = ix.rescore_device([mike, zulu, kilo], [0, 3], d_all[1], d_all[0], model="bm25", order=1, m=4, k1=0.3, b=0.2)
    got = _fetch_result(sme, r, 1)
    ref = RR.Ref(R.Ref.from_csr(ix.csr()), ix.weights())
    _same(got, ref.run([([mike, zulu, kilo], pall[1])], "bm25", 1, 4, 0, 0.3, 0.2))
    ix.rescore([mike], [0, 1], pall[1], pall[0], model="tfidf")
    # the last Boolean, phrase and BM25 results as they were
    assert np.array_equal(_fetch(sme, d_b[1], d_b[3], np.int32), b[1]) and len(b[1]) == 5
    assert _fetch(sme, d_b[2], d_b[3], np.float64).tobytes() == b[2].tobytes()
    assert np.array_equal(_fetch(sme, d_all[1], d_all[4], np.int32), pall[1]) and d_all[4] == len(pall[1]) > 6
    assert np.array_equal(p[1], pall[1][:6]) and d_p[4] == 6
    assert ix.query_bm25_stats() == bm_stats
    again = ix.query_bm25(ids, qoff, 8)
    assert again[0].tobytes() == bm[0].tobytes() and again[1].tobytes() == bm[1].tobytes()
    # and the other way round: the rescore result outlives the other features' calls
    r = ix.rescore_device([mike, zulu], [0, 2], d_all[1], d_all[0], model="tfidf", order=1, m=9)
    want = _fetch_result(sme, r, 1)
    ix.query_boolean(bq)
    ix.query_phrase([[lima, zulu]])
    ix.query_near([([kilo], 1, True)])
    ix.query_bm25(ids, qoff, 3)
    _same(_fetch_result(sme, r, 1), want)
    assert len(want[1]) == 9


# ---- refusals ------------------------------------------------------------------------------------
def _raises(sme, call, code, *words):
    with pytest.raises(sme.SmeError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_candidates_not_strictly_ascending(sme, crafted):
    ix, ref, n, T = crafted
    ok = ([A], list(range(1, 2 * T + 2)))
    empty = {"candidates": 0, "found": 0, "matches": 0, "tile": T}
    cases = []
    for at, kind in ((5, "equal"), (700, "descending"), (T, "equal"), (T, "descending"), (2 * T, "descending")):
        docs = list(ok[1])  # candidates at - 1 and at: the last of a tile and the first of the next for at = T, 2 T
        if kind == "equal":
            docs[at] = docs[at - 1]
        else:
            docs[at - 1], docs[at] = docs[at], docs[at - 1]
        cases.append(docs)
    cases.append([7, LO])  # signed order: the smallest int32 after a positive docno descends
    for docs in cases:
        assert not np.all(np.diff(np.asarray(docs, np.int64)) > 0)
        queries = [ok, ([C_], docs), ok]
        ids, qoff, dd, doff = RR.batch(queries)
        ix.rescore(*RR.batch([ok]), model="bm25")
        assert ix.rescore_stats()["candidates"] == len(ok[1])
        _raises(sme, lambda: ix.rescore(ids, qoff, dd, doff, model="bm25"), SME_EINVAL, "ascending", "query 1")
        assert ix.rescore_stats() == empty  # the previous result reads as empty
        ix.rescore(*RR.batch([ok]), model="tfidf")
        with _on_device(sme, dd, doff) as (d_docs, d_doff):
            _raises(sme, lambda: ix.rescore_device(ids, qoff, d_docs, d_doff, model="tfidf"), SME_EINVAL, "ascending",
                    "query 1")
        assert ix.rescore_stats() == empty
    # a query's last candidate above the next query's first is no fault
    two = [([A], [9, 10]), ([A], [1, 2])]
    _same(ix.rescore(*RR.batch(two), model="bm25"), ref.run(two, "bm25"))
    ids, qoff, dd, doff = RR.batch(two)
    with _on_device(sme, dd, doff) as (d_docs, d_doff):
        _same(_fetch_result(sme, ix.rescore_device(ids, qoff, d_docs, d_doff, model="bm25"), 2), ref.run(two, "bm25"))


def test_limits_and_arguments(sme, crafted):
    ix, ref, n, T = crafted
    docs, doff = [1, 2, 3], [0, 1, 2, 3]
    ids, qoff = R.batch([[A], [GAP] * 1025, [C_]])
    _raises(sme, lambda: ix.rescore(ids, qoff, docs, doff), SME_ELIMIT, "query 1")
    three = [([A], [1]), ([GAP] * 1024, [2]), ([C_], [3])]  # the limit itself, and the next valid call
    _same(ix.rescore(*RR.batch(three)), ref.run(three, "bm25"))
    _raises(sme, lambda: ix.rescore([A], [0, 1], [1], [0, 2 ** 31]), SME_ELIMIT, "2^31")  # (refused before a docno is read)
    _raises(sme, lambda: ix.rescore([A], [0, 2 ** 31], [1], [0, 1]), SME_ELIMIT, "2^31")
    for k1, b in ((float("nan"), 0.75), (-0.5, 0.75), (float("inf"), 0.75), (1.2, 1.5), (1.2, -0.1), (1.2, float("nan"))):
        _raises(sme, lambda: ix.rescore([A], [0, 1], [1], [0, 1], model="bm25", k1=k1, b=b), SME_EINVAL, "k1")
        one = ix.rescore([A], [0, 1], [1], [0, 1], model="tfidf", k1=k1, b=b)  # TF-IDF does not read them
        assert one[1].tolist() == [1]
    L = sme.lib()
    outs = [C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()]
    keep, p = sme.Index._typed_ptrs([[A], [0, 1], [1], [0, 1]], (np.int32, np.int64, np.int32, np.int64))

    def raw(model=1, min_hits=0, order=1, m=0, nq=1):
        return L.sme_query_rescore(ix._h, *p, nq, model, 1.2, 0.75, min_hits, order, m, *[C.byref(o) for o in outs])

    assert raw() == 0 and outs[1][0] == 1
    for kw, word in (({"model": 2}, b"model"), ({"model": -1}, b"model"), ({"order": 2}, b"order"),
                     ({"order": -1}, b"order"), ({"m": -1}, b"m must"), ({"min_hits": -1}, b"min_hits"),
                     ({"nq": -1}, b"nq")):
        assert raw(**kw) == SME_EINVAL and word in L.sme_last_error(), (kw, L.sme_last_error())
    with pytest.raises(ValueError):
        ix.rescore([A], [0, 1], [1], [0, 1], model="bm26")
    _raises(sme, lambda: ix.rescore([A, ix.V], [0, 1, 2], [1, 2], [0, 1, 2]), SME_EINVAL, "term id", "query 1")
    _raises(sme, lambda: ix.rescore([A, -2], [0, 2], [1], [0, 1]), SME_EINVAL, "term id", "query 0")
    _raises(sme, lambda: ix.rescore([A, C_], [0, 2, 1], [1, 2], [0, 1, 2]), SME_EINVAL, "q_offsets")
    _raises(sme, lambda: ix.rescore([A, C_], [1, 2], [1], [0, 1]), SME_EINVAL, "q_offsets")
    _raises(sme, lambda: ix.rescore([A, C_], [0, 1, 2], [1, 2], [0, 2, 1]), SME_EINVAL, "d_offsets", "query 1")
    _raises(sme, lambda: ix.rescore([A], [0, 1], [1], [1, 1]), SME_EINVAL, "d_offsets")
    dd, do = np.array([1, 2], np.int32), np.array([0, 2, 1], np.int64)
    with _on_device(sme, dd, do) as (d_docs, d_doff):
        _raises(sme, lambda: ix.rescore_device([A, C_], [0, 1, 2], d_docs, d_doff), SME_EINVAL, "d_offsets", "query 1")
    _raises(sme, lambda: ix.ctx.set_option("rescore_path", 3), SME_EINVAL)
    _raises(sme, lambda: ix.ctx.set_option("rescore_path", -1), SME_EINVAL)
    _same(ix.rescore(*RR.batch(three)), ref.run(three, "bm25"))  # the index answers as before


def test_no_query_side(sme, built):
    """A chargram output and a records-only index (merged shard pieces) have no postings by
    document: SME_EINVAL from both entries, with and without queries, as the query entries
    refuse them."""
    import torch
    grams = sme.Context(2, 2).build_chargram(b"<DOC>\n<DOCNO> X-1 </DOCNO>\n<TEXT>\nalpha beta\n</TEXT>\n</DOC>\n")
    ix = built[0]
    sizes = ix.pack_pieces(1)
    blob = torch.empty(max(sum(sizes), 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ix.pack_pieces(1, blob.data_ptr())
    merged = ix.ctx.merge_pieces(blob.data_ptr(), sizes)
    L = sme.lib()
    outs = [C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()]
    dd, do = np.array([1, 2], np.int32), np.array([0, 2], np.int64)
    with _on_device(sme, dd, do) as (d_docs, d_doff):
        for obj, word in ((grams, "CharKGramTermIndexer"), (merged, "records-only")):
            assert L.sme_query_rescore(obj._h, None, None, None, None, 0, 1, 1.2, 0.75, 0, 1, 0,
                                       *[C.byref(o) for o in outs]) == SME_EINVAL
            assert word.encode() in L.sme_last_error()
            _raises(sme, lambda: sme.Index.rescore(obj, [0], [0, 1], dd, do), SME_EINVAL, word)
            _raises(sme, lambda: sme.Index.rescore_device(obj, [0], [0, 1], d_docs, d_doff), SME_EINVAL, word)
            _raises(sme, lambda: sme.Index.rescore_device(obj, [], [0], 0, 0), SME_EINVAL, word)
        assert sme.Index.rescore(ix, [0], [0, 1], dd, do)[0].tolist() == [0, 2]  # the built index answers


# ---- a built index: negative docnos, duplicates, docno 0 ------------------------------------------
@pytest.fixture(scope="module")
def built(sme):
    corpus, mapping = common.fuzz_corpus(8, 120, extra_docids=40)
    ctx = sme.Context(1, 3, 1)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(mapping))
    ix = ctx.build(corpus)
    return ix, RR.Ref(R.Ref.from_csr(ix.csr()), ix.weights())


@pytest.mark.parametrize("model,k1,b", MODELS[:2] + MODELS[-1:])
def test_built_negative_docnos(built, model, k1, b):
    ix, ref = built
    bm = ref.bm
    assert bm.dmin < 0
    rng = random.Random(5)
    by_df = sorted(range(bm.V), key=lambda t: -int(bm.df[t]))
    every = list(range(bm.dmin - 3, bm.dmin + bm.span + 3))
    queries = []
    for i in range(40):
        pool = by_df[:20] if rng.random() < 0.5 else range(bm.V)
        slots = [rng.choice(pool) for _ in range(rng.randint(1, 8))]
        cands = every if i % 4 == 0 else sorted(rng.sample(every, rng.randint(1, len(every))))
        queries.append((slots, cands))
    for path in PATHS:
        ix.ctx.set_option("rescore_path", path)
        try:
            for order, m, min_hits in ((1, 10, 1), (0, 0, 0), (1, 0, 2)):
                _same(ix.rescore(*RR.batch(queries), model=model, order=order, m=m, min_hits=min_hits, k1=k1, b=b),
                      ref.run(queries, model, order, m, min_hits, k1, b))
        finally:
            ix.ctx.set_option("rescore_path", 0)


# ---- the facade ---------------------------------------------------------------------------------------
def test_facade(sme):
    corpus, mapping, st = TQ._craft()
    ix = TQ._ctx(sme, mapping, 1, 0).build(corpus)
    fw = sme.IntDocVectorsForwardIndex(ix, mapping)
    ref = RR.Ref(R.Ref.from_csr(ix.csr()), ix.weights())
    kilo, lima, mike, nova, oscar, zulu = TQ._words(ix, "kilo", "lima", "mike", "nova", "oscar", "zulu")

    def ranked(matches, slots, scorer, k, k1=1.2, b=0.75):
        return ref.rank(slots, matches, scorer, 1, k, 0, k1, b)[0].tolist()

    # Boolean
    groups = fw.get_boolean(["zul*", "mike", "-quebec", "kilo"])
    slots = [t for ids, ex in groups if not ex for t in ids]
    assert len(slots) >= 4 and any(ex for _, ex in groups)
    assert fw.rank_boolean(7) == ix.query_boolean([groups], 1, 7)[1].tolist() == fw.rank_boolean(7, None)
    matches = ix.query_boolean([groups], 0, 0)[1]
    assert len(matches) > 10
    assert fw.rank_boolean(7, "bm25") == ranked(matches, slots, "bm25", 7)
    assert fw.rank_boolean(5, scorer="bm25", k1=0.4, b=1.0) == ranked(matches, slots, "bm25", 5, 0.4, 1.0)
    assert fw.rank_boolean(500, "tfidf") == ranked(matches, slots, "tfidf", 500) and len(matches) < 500
    # phrase
    assert fw.get_phrase("the kilo of lima") == [kilo, lima]
    assert fw.rank_phrase(6) == ix.query_phrase([[kilo, lima]], 1, 6)[1].tolist()
    matches = ix.query_phrase([[kilo, lima]], 0, 0)[1]
    assert fw.rank_phrase(6, "bm25") == ranked(matches, [kilo, lima], "bm25", 6)
    assert fw.rank_phrase(6, "tfidf", 9.0, 0.1) == ranked(matches, [kilo, lima], "tfidf", 6)
    fw.get_phrase("kilo xylophone")
    assert fw.rank_phrase(6, "bm25") == [] == fw.rank_phrase(6)
    # proximity
    near = fw.get_near("oscar nova", 3, ordered=False)
    assert fw.rank_near(4) == ix.query_near([near], 1, 4)[1].tolist()
    matches = ix.query_near([near], 0, 0)[1]
    assert len(matches) > 4 and fw.rank_near(4, "bm25", 2.0, 0.0) == ranked(matches, near[0], "bm25", 4, 2.0, 0.0)
    # structured: the term ids of all leaves of the required groups, in listed order
    sq = fw.get_structured('"kilo lima" mike|nova -#uw:3(nova oscar) zulu')
    slots = [t for leaves, ex in sq if not ex for ids, _, _ in leaves for t in ids]
    assert slots == [kilo, lima, mike, nova, zulu]
    assert fw.rank_structured(8) == ix.query_structured([sq], 1, 8)[1].tolist()
    matches = ix.query_structured([sq], 0, 0)[1]
    assert len(matches) > 8 and fw.rank_structured(8, "bm25") == ranked(matches, slots, "bm25", 8)
    assert fw.rank_structured(8, "tfidf") == ranked(matches, slots, "tfidf", 8)
    with pytest.raises(ValueError):
        fw.rank_boolean(3, "bm26")
