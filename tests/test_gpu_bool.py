"""Boolean retrieval on the device (sme_query_boolean*): every result is held to
the restatement of bool_ref.py over the index's own query-side CSR
(Index.weights()) -- offsets, docnos and the bits of every score exactly equal,
which includes the order and the cut -- on an index loaded from hand-written
record streams whose posting lists sit on the kernel's chunk, round and wave
edges, and on a built index, where a one-group query is also held to
sme_query_topk."""
import functools
import random

import numpy as np
import pytest

import bool_ref as B
import common
import load_streams as S

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
NDOCS = 700
REQ, EXC = False, True

# the crafted lists: term i = "t%02d", tf of its posting in document d = 1 + (7 d + i) % 5
LISTS = [
    list(range(1, NDOCS + 1)),      # ALL
    list(range(2, NDOCS + 1, 2)),   # E2: every 2nd
    list(range(3, NDOCS + 1, 3)),   # E3: every 3rd
    list(range(1, 64)),             # F63 .. F257: the first n documents
    list(range(1, 65)),
    list(range(1, 66)),
    list(range(1, 256)),
    list(range(1, 257)),
    list(range(1, 258)),
    list(range(600, NDOCS + 1)),    # HI
    list(range(1, 51)),             # LO
    [333],                          # ONE
    [],                             # NONE: a term without a posting
]
ALL, E2, E3, F63, F64, F65, F255, F256, F257, HI, LO, ONE, NONE = range(13)

QUERIES = [
    # single terms: lists ending on, one short of and one past 64 and 256 candidates
    [([ALL], REQ)], [([F63], REQ)], [([F64], REQ)], [([F65], REQ)], [([F255], REQ)], [([F256], REQ)], [([F257], REQ)],
    [([ONE], REQ)], [([NONE], REQ)],
    # two- and three-group AND
    [([E2], REQ), ([E3], REQ)], [([ALL], REQ), ([F65], REQ)], [([ALL], REQ), ([E2], REQ), ([E3], REQ)],
    [([F257], REQ), ([E3], REQ), ([F64], REQ)], [([ONE], REQ), ([ALL], REQ)], [([ALL], REQ), ([ONE], REQ), ([E3], REQ)],
    # OR-groups; a driver group whose slots overlap emits a document once
    [([E2, E3], REQ)], [([F63, F65, F64], REQ), ([E2], REQ)], [([HI, LO], REQ), ([E3, ONE], REQ)],
    [([F256, F64, F257], REQ)], [([E3, ALL, E2], REQ), ([F65, HI], REQ)],
    # exclusions
    [([ALL], REQ), ([E2], EXC)], [([ALL], REQ), ([E2, E3], EXC)], [([F257], REQ), ([F255], EXC)],
    [([ALL], REQ), ([ONE], EXC)], [([E2], REQ), ([E3], EXC), ([LO], EXC)], [([E2], EXC), ([ALL], REQ)],
    # unknown terms, empty groups, queries that match nothing by their structure
    [([-1, E3], REQ), ([ALL, -1], REQ)], [([E2], REQ), ([-1], EXC)], [([-1], REQ)], [([E2], REQ), ([-1], REQ)],
    [([E2], REQ), ([], REQ)], [([E2], REQ), ([], EXC)], [([E2], EXC)], [([E2], EXC), ([], EXC)], [],
    [([ALL], REQ), ([NONE], REQ)], [([ALL, NONE], REQ)], [([ALL], REQ), ([NONE], EXC)],
    # the same term required and excluded
    [([E3], REQ), ([E3], EXC)], [([E2, E3], REQ), ([E3], EXC)],
    # a term repeated in a group and across groups counts twice in the score
    [([E3, E3], REQ), ([E3], REQ)], [([E2, E3, E2], REQ)], [([F65], REQ), ([F65, F65], REQ), ([ALL], REQ)],
    # lists disjoint from the chunk's docno range, below and above it
    [([HI], REQ), ([LO], REQ)], [([ALL], REQ), ([HI], REQ)], [([ALL], REQ), ([LO], REQ)],
    [([ALL], REQ), ([LO], EXC)], [([ALL], REQ), ([HI], EXC)], [([ALL], REQ), ([HI, LO], REQ)],
    [([E2], REQ), ([HI], REQ), ([LO], EXC)],
    # more slots than threads stage per pass, and the limits themselves: 1024 slots, 64 groups
    [([E2] * 300 + [E3] * 300, REQ), ([F257], REQ)], [([E3] * 16, REQ)] * 64,
    [([F65] * 1000 + [-1] * 23, EXC), ([ALL], REQ)],
]


def _tf(d, i):
    return 1 + (7 * d + i) % 5


def _crafted(sme, idf_mode=1):
    recs = []
    for i, docs in enumerate(LISTS):
        posts = sorted(((d, _tf(d, i)) for d in docs), key=lambda p: (-p[1], p[0]))  # (tf desc, docno asc)
        recs.append(S.record(b"t%02d" % i, posts))
    body = b"".join(recs)
    ix = sme.Context(1, 1, idf_mode).load_records([body, S.counter(S.counter_posts(list(range(1, NDOCS + 1))))])
    assert ix.V == len(LISTS) and ix.N == NDOCS
    return ix


def _ref_of(ix):
    off, dn, w = ix.weights()
    for t in range(ix.V):
        assert np.all(np.diff(dn[off[t]:off[t + 1]]) > 0)  # docno ascending, as the restatement assumes
    return B.Ref(off, dn, w)


@pytest.fixture(scope="module")
def crafted(sme):
    ix = _crafted(sme)
    ref = _ref_of(ix)
    assert [ref.count(t) for t in range(ix.V)] == [len(x) for x in LISTS]
    assert len(set(ref.w)) > 10  # the weights differ
    return ix, ref, {}


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]), np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:8]
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:8]
    assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64)), np.nonzero(got[2] != want[2])[0][:8]


def _check(ix, ref, queries, order, m, first_driver=False, cache=None, key=None):
    """One batch against the restatement, the call's counts included."""
    got = ix.query_boolean(queries, order, m)
    k = (key, order, m, first_driver)
    if cache is None or key is None or k not in cache:
        want = ref.run(queries, order, m, first_driver)
        if cache is not None and key is not None:
            cache[k] = want
    else:
        want = cache[k]
    _same(got, want[0])
    assert ix.boolean_stats() == (want[1], want[2])
    return got


def test_crafted_answers(crafted):
    """A few results written out by hand, so the restatement is not the only witness."""
    ix, ref, _ = crafted
    off, dn, sc = ix.query_boolean([[([F257], REQ), ([F255], EXC)], [([HI], REQ), ([LO], REQ)], [],
                                    [([F65], REQ), ([E2], EXC), ([E3], EXC)]], 0, 0)
    assert off.tolist() == [0, 2, 2, 2, 24]
    assert dn[:2].tolist() == [256, 257] and dn[2:].tolist() == [d for d in range(1, 66) if d % 2 and d % 3]
    _, _, w = ix.weights()
    o = ix.offsets()
    assert sc[0] == w[o[F257] + 255] and sc[1] == w[o[F257] + 256]
    assert ix.boolean_stats() == (257 + 50 + 65, 24)


@pytest.mark.parametrize("driver", [0, 1])
@pytest.mark.parametrize("chunk", [64, 128, 1024])
def test_crafted_queries(crafted, chunk, driver):
    ix, ref, cache = crafted
    ix.ctx.set_option("bool_chunk", chunk)
    ix.ctx.set_option("bool_driver", driver)
    try:
        for order in (0, 1):
            for m in (0, 1, 10, 1000):
                off, dn, sc = _check(ix, ref, QUERIES, order, m, bool(driver), cache, "Q")
                if m == 0 and order == 0:
                    whole = (off, dn, sc)
        # the queries reach what they are meant to reach
        off, dn, sc = whole
        n = np.diff(off)
        assert n[0] == NDOCS and n[1:7].tolist() == [63, 64, 65, 255, 256, 257] and n[9] == NDOCS // 6
        assert n[QUERIES.index([])] == 0 and n[QUERIES.index([([HI], REQ), ([LO], REQ)])] == 0
        assert n[QUERIES.index([([E2, E3], REQ)])] == NDOCS // 2 + NDOCS // 3 - NDOCS // 6
        # every query as a batch of its own
        if chunk == 64:
            for i, q in enumerate(QUERIES):
                o1, d1, s1 = ix.query_boolean([q], 0, 0)
                assert o1.tolist() == [0, n[i]] and np.array_equal(d1, dn[off[i]:off[i + 1]]), i
                assert s1.tobytes() == sc[off[i]:off[i + 1]].tobytes(), i
    finally:
        ix.ctx.set_option("bool_chunk", 1024)
        ix.ctx.set_option("bool_driver", 0)


def test_driver_choice_shows_in_the_counts(crafted):
    ix, ref, _ = crafted
    q = [[([ALL], REQ), ([F65], REQ)]]
    ix.query_boolean(q)
    assert ix.boolean_stats() == (65, 65)  # the smaller group drove
    ix.ctx.set_option("bool_driver", 1)
    try:
        ix.query_boolean(q)
        assert ix.boolean_stats() == (NDOCS, 65)
        ix.query_boolean([[([NONE], REQ), ([ALL], REQ)], [([ALL], REQ), ([NONE], REQ)]])
        assert ix.boolean_stats() == (0, 0)  # a query that cannot match is not searched
    finally:
        ix.ctx.set_option("bool_driver", 0)


@functools.lru_cache(maxsize=None)
def _fuzz():
    return common.fuzz_corpus(8, 120)


def _built(sme, idf_mode):
    corpus, ids = _fuzz()
    ctx = sme.Context(1, 3, idf_mode, tiebreak=sme.SME_TIE_DOCNO)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    return ctx.build(corpus)


def _random_queries(rng, V, n):
    qs = []
    for _ in range(n):
        groups = []
        for _ in range(rng.randint(0, 4)):
            ids = [rng.randrange(-1, V) for _ in range(rng.randint(0, 5))]
            groups.append((ids, rng.random() < 0.25))
        qs.append(groups)
    return qs


@pytest.mark.parametrize("idf_mode", [0, 1])
def test_built_index_against_topk(sme, idf_mode):
    ix = _built(sme, idf_mode)
    ref = _ref_of(ix)
    rng = random.Random(5 + idf_mode)
    df = np.diff(ix.offsets())
    common_terms = [int(t) for t in np.argsort(-df, kind="stable")[:40]]
    flat = [[rng.choice(common_terms) for _ in range(rng.randint(1, 6))] for _ in range(10)]
    flat += [[rng.randrange(ix.V) for _ in range(rng.randint(1, 8))] + [-1] for _ in range(6)]
    flat.append(common_terms[:3] + common_terms[:2])  # duplicates count twice
    terms = np.array([t for q in flat for t in q], np.int32)
    qoff = np.cumsum([0] + [len(q) for q in flat]).astype(np.int64)
    queries = [[(q, REQ)] for q in flat]
    for k in (10, 100):
        dn, sc = ix.query_topk(terms, qoff, k)
        off, bd, bs = _check(ix, ref, queries, 1, k)
        for i in range(len(flat)):
            # query_topk's pads (docno -1, score 0) cut off; documents outside the
            # mapping have negative docnos of their own, far from -1
            n = int((~((dn[i] == -1) & (sc[i] == 0.0))).sum())
            assert off[i + 1] - off[i] == n and np.array_equal(bd[off[i]:off[i + 1]], dn[i, :n]), (i, k)
            assert bs[off[i]:off[i + 1]].tobytes() == sc[i, :n].tobytes(), (i, k)
        assert np.diff(off).max() == k if k == 10 else np.diff(off).max() > 10
    # structured queries over the same index; its docnos include negative ones
    # (documents outside the mapping), so docno order is signed order
    assert ix.weights()[1].min() < -1
    qs =_random_queries(rng, ix.V, 60) + [[(common_terms[:8], REQ), (common_terms[8:16], REQ)],
                                           [(common_terms[:20], REQ), (common_terms[20:24], EXC)]]
    for order, m in ((0, 0), (1, 0), (1, 3)):
        off, _, _ = _check(ix, ref, qs, order, m)
    assert off[-1] > 20
    ix.ctx.set_option("bool_driver", 1)
    ix.ctx.set_option("bool_chunk", 64)
    _check(ix, ref, qs, 1, 0, True)


def test_after_reweight(sme):
    ix = _crafted(sme)
    qs = QUERIES[:24]
    before = _check(ix, _ref_of(ix), qs, 1, 10)
    ix.reweight(3 * ix.N)
    after = _check(ix, _ref_of(ix), qs, 1, 10)  # the restatement over the new weights
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[2], after[2])
    ix.reweight(ix.N)
    _same(ix.query_boolean(qs, 1, 10), before)


def test_device_entry(sme, crafted):
    ix, ref, _ = crafted
    for qs, order, m in ((QUERIES, 0, 0), (QUERIES, 1, 10), ([[([HI], REQ), ([LO], REQ)]], 0, 0), ([], 1, 0)):
        off, dn, sc = ix.query_boolean(qs, order, m)
        d_off, d_dn, d_sc, total = ix.query_boolean_device(qs, order, m)
        assert total == off[-1] and d_off
        got_off = np.zeros(len(qs) + 1, np.int64)
        sme.memcpy(got_off.ctypes.data, d_off, got_off.nbytes)
        got_dn, got_sc = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.float64)
        if total:
            sme.memcpy(got_dn.ctypes.data, d_dn, 4 * total)
            sme.memcpy(got_sc.ctypes.data, d_sc, 8 * total)
        _same((got_off, got_dn[:total], got_sc[:total]), (off, dn, sc))


def test_buffers_are_independent(sme):
    ix = _built(sme, 0)
    qs = [[([t], REQ)] for t in range(0, ix.V, 7)]
    pats = ["a*", "*ing", "run*"]
    w_off, w_ids = ix.expand_wildcards(pats)
    dw_off, dw_ids, w_total = ix.expand_wildcards_device(pats)
    b_off, b_dn, b_sc = ix.query_boolean(qs, 1, 0)  # a Boolean call leaves the expansion alone
    got = np.zeros(w_total, np.int32)
    sme.memcpy(got.ctypes.data, dw_ids, 4 * w_total)
    got_off = np.zeros(len(pats) + 1, np.int64)
    sme.memcpy(got_off.ctypes.data, dw_off, got_off.nbytes)
    assert w_total > 0 and np.array_equal(got, w_ids) and np.array_equal(got_off, w_off)
    d_off, d_dn, d_sc, total = ix.query_boolean_device(qs, 1, 0)
    ix.expand_wildcards(["*", "b*"])  # and the other way round
    ix.suggest_terms(["runing"], 2, 5)
    got_off = np.zeros(len(qs) + 1, np.int64)
    got_dn, got_sc = np.zeros(total, np.int32), np.zeros(total, np.float64)
    sme.memcpy(got_off.ctypes.data, d_off, got_off.nbytes)
    sme.memcpy(got_dn.ctypes.data, d_dn, 4 * total)
    sme.memcpy(got_sc.ctypes.data, d_sc, 8 * total)
    assert total > 0
    _same((got_off, got_dn, got_sc), (b_off, b_dn, b_sc))


def _raises(call, code, word=None):
    with pytest.raises(Exception) as e:
        call()
    assert getattr(e.value, "code", None) == code, str(e.value)
    if word is not None:
        assert word in str(e.value), str(e.value)


def test_errors(sme, crafted):
    ix, ref, _ = crafted
    ok = [[([E2], REQ), ([E3], REQ)]]
    before = ix.query_boolean(ok, 0, 0)
    i32, i64, u8 = np.int32, np.int64, np.uint8
    for entry in (ix.query_boolean, ix.query_boolean_device):
        # the limits name the query
        _raises(lambda: entry(ok + [[([E2], REQ)] * 65]), SME_ELIMIT, "query 1")
        _raises(lambda: entry(ok + ok + [[([E2] * 1000, REQ), ([E3] * 25, EXC)]]), SME_ELIMIT, "query 2")
        _raises(lambda: entry(ok, 0, -1), SME_EINVAL)
        for order in (2, -1):
            _raises(lambda: entry(ok, order, 0), SME_EINVAL)
        # term ids outside [-1, V)
        _raises(lambda: entry(ok + [[([E2, ix.V], REQ)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([[([-2], EXC)]] + ok), SME_EINVAL, "query 0")
        # a flag other than 0 / 1
        _raises(lambda: entry([[([E2], 2)]]), SME_EINVAL)
        _raises(lambda: entry(ok + [[([E2], REQ), ([E3], 255)]]), SME_EINVAL)
        # offsets not ascending, not from 0, or not agreeing
        t, g, f = np.array([E2, E3, E2], i32), np.array([0, 1, 2, 3], i64), np.zeros(3, u8)
        entry(None, arrays=(t, g, f, np.array([0, 1, 3], i64)))
        for qo in ([0, 2, 1, 3], [1, 2, 3], [-1, 1, 3], [0, 3, 2]):
            _raises(lambda: entry(None, arrays=(t, g, f, np.array(qo, i64))), SME_EINVAL)
        for go in ([0, 2, 1, 3], [1, 1, 2, 3], [0, 1, 3, 2], [0, -1, 2, 3]):
            _raises(lambda: entry(None, arrays=(t, np.array(go, i64), f, np.array([0, 1, 3], i64))), SME_EINVAL)
    _raises(lambda: ix.query_boolean(None, arrays=(t, g, f, np.array([0, 2, 1, 3], i64))), SME_EINVAL, "query 1")
    for name, bad in (("bool_chunk", 0), ("bool_chunk", 63), ("bool_chunk", 100), ("bool_chunk", 4160),
                      ("bool_driver", 2), ("bool_driver", -1)):
        _raises(lambda: ix.ctx.set_option(name, bad), SME_EINVAL)
    for good in (64, 4096, 1024):
        ix.ctx.set_option("bool_chunk", good)
    # the limits themselves are accepted (QUERIES holds them); nq == 0 is valid
    off, dn, sc = ix.query_boolean([], 1, 5)
    assert off.tolist() == [0] and dn.size == 0 and sc.size == 0 and ix.boolean_stats() == (0, 0)
    _same(ix.query_boolean(ok, 0, 0), before)


def test_match_limit(sme):
    """2^31 or more matches in a batch before the cut are SME_ELIMIT, decided after
    the count pass; the largest batch below the limit is answered.  One-group
    [ALL] queries match all 700 documents each: 3,067,834 of them give 2^31 + 152
    matches, one fewer 2^31 - 548.  An index and context of its own, closed at the
    end, so the call's pooled device blocks go back to the device."""
    nq = -(-(1 << 31) // NDOCS)
    assert (nq - 1) * NDOCS < 1 << 31 <= nq * NDOCS
    ix = _crafted(sme)
    try:
        def arrays(n):
            return (np.full(n, ALL, np.int32), np.arange(n + 1, dtype=np.int64), np.zeros(n, np.uint8),
                    np.arange(n + 1, dtype=np.int64))
        _raises(lambda: ix.query_boolean(None, 0, 1, arrays=arrays(nq)), SME_ELIMIT, "2^31")
        _raises(lambda: ix.query_boolean_device(None, 1, 0, arrays=arrays(nq)), SME_ELIMIT, "2^31")
        off, dn, sc = ix.query_boolean(None, 0, 1, arrays=arrays(nq - 1))
        assert ix.boolean_stats() == ((nq - 1) * NDOCS, (nq - 1) * NDOCS)
        o, d, w = ix.weights()
        assert d[o[ALL]] == 1  # every query's first document by docno, with its weight
        assert np.array_equal(off, np.arange(nq, dtype=np.int64))
        assert dn.size == nq - 1 and np.all(dn == 1)
        assert np.all(sc.view(np.int64) == w[o[ALL]:o[ALL] + 1].view(np.int64)[0])
    finally:
        ctx = ix.ctx
        ix.close()
        ctx.close()


def test_indexes_without_a_query_side(sme):
    import torch
    corpus, ids = _fuzz()
    built = _built(sme, 0)
    cg = sme.Context(2, 2).build_chargram(corpus)
    sizes = built.pack_pieces(1)
    blob = torch.empty(max(sum(sizes), 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    built.pack_pieces(1, blob.data_ptr())
    merged = built.ctx.merge_pieces(blob.data_ptr(), sizes)
    q = [[([0], REQ)]]
    for obj in (cg, merged):
        _raises(lambda: sme.Index.query_boolean(obj, q), SME_EINVAL)
        _raises(lambda: sme.Index.query_boolean_device(obj, q), SME_EINVAL)
    assert sme.Index.query_boolean(built, q)[0][-1] > 0
    # K = 2: the ids are gram ids
    ctx2 = sme.Context(2, 2)
    ctx2.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    k2 = ctx2.build(corpus)
    rng = random.Random(11)
    qs = _random_queries(rng, k2.V, 30) + [[([g], REQ)] for g in range(0, k2.V, max(k2.V // 20, 1))]
    off, _, _ = _check(k2, _ref_of(k2), qs, 1, 0)
    assert off[-1] > 0


DOCS = ["compact network java", "compass network", "compile networks python", "network java", "compact compass",
        "java compile network network", "the network", "python compass java", "compose networking"]


def test_facade(sme):
    ids = ["D%02d" % i for i in range(1, len(DOCS) + 1)]
    corpus = "".join("<DOC>\n<DOCNO> %s </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (d, t)
                     for d, t in zip(ids, DOCS)).encode()
    ctx = sme.Context(1, 2, 1)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    ix = ctx.build(corpus)
    ref = _ref_of(ix)
    fw = sme.IntDocVectorsForwardIndex(ix)
    net, java = (int(t) for t in ix.lookup(ctx.process_content("network java")))
    assert net >= 0 and java >= 0

    def want(groups, k):
        (_, dn, _), _, _ = ref.run([groups], 1, k)
        return dn.tolist()

    groups = fw.get_boolean(["COMP*", "network", "-java"])
    assert len(groups) == 3 and len(groups[0][0]) >= 4 and groups[1:] == [([net], False), ([java], True)]
    assert [flag for _, flag in groups] == [False, False, True]
    got = fw.rank_boolean(10)
    assert got == want(groups, 10) and got
    # document 2 holds "compass network"; 1, 4, 6 and 8 hold "java", 5 and 7 lack one of the two
    assert 2 in got and not {1, 4, 5, 6, 7, 8} & set(got)
    assert fw.rank_boolean(1) == got[:1]
    # a stopword is dropped, an unknown required word gives nothing, an unknown excluded one changes nothing
    assert fw.get_boolean(["the", "network"]) == [([net], False)]
    assert {1, 2, 4, 6, 7} <= set(fw.rank_boolean(10)) and fw.rank_boolean(10) == want([([net], False)], 10)
    assert fw.get_boolean(["network", "zzzzqq"]) == [([net], False), ([-1], False)] and fw.rank_boolean() == []
    assert fw.get_boolean(["network", "-zzzzqq"])[1] == ([-1], True)
    assert fw.rank_boolean(20) == want([([net], False)], 20)
    assert fw.get_boolean(["-java"]) == [([java], True)] and fw.rank_boolean() == []
    assert fw.get_boolean(["nosuch*", "network"])[0] == ([], False) and fw.rank_boolean() == []
    # the other query calls are untouched by the groups
    fw.getValue(ctx.process_content("java"))
    assert fw.rank(10) == want([([java], False)], 10)
