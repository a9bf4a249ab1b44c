"""Proximity queries on the device (sme_query_near*): the ordered window #od:N and the
unordered window #uw:N over the positions a K = 1 build keeps ("positions" 1).
Every docno, freq and score is held to near_ref.py, the brute-force restatement
(itself held to the oracle chain by test_near_ref.py): docnos and freqs exactly,
scores bit for bit.  Where code exists that answers the same question -- ordered
N = 1 is the phrase, unordered N = 2^31 - 1 on one-record documents is Boolean AND
-- the answers are held to that code too.  No tolerance anywhere."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import near_ref as NR
import oracle_lib as O
import phrase_ref as P
import test_gpu_phrase as TP  # (its corpora and helpers; nothing of it is changed)

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
MAXN = 2 ** 31 - 1
ORDERS = ((0, 0), (1, 0), (1, 3), (0, 1))
_ctx, _same, _raises, _doc = TP._ctx, TP._same, TP._raises, TP._doc

A, B, Cw, FILL = "kilo", "lima", "mike", "zulu"
D32 = ["w%03d" % (7 * j + 3) for j in range(32)]  # 32 distinct terms
LENS = (1, 2, 5, 32)
STREAM_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 257)


def _q(ix, queries):
    """Queries (terms as strings or None, width, ordered) -> the same with term ids."""
    words = sorted({t for q in queries for t in q[0] if t is not None})
    table = dict(zip(words, ix.lookup(words).tolist())) if words else {}
    return [([-1 if t is None else table[t] for t in q[0]], q[1], q[2]) for q in queries]


# ---- 1. the edge corpus ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge():
    """(corpus, mapping, queries as (text, width, ordered), {case name: record index}).
    One case per record.  A record with its DOCNO last has the body at stream
    position 0 (the DOCNO's two tokens end the stream); one without DOCNO is the
    body alone, under docno 0."""
    docs, ids, queries, case = [], [], [], {}
    n = [0]

    def add(body, docid="new", mapped=True, docno_last=False, name=None):
        if docid == "new":
            n[0] += 1
            docid = "ED%06d-%02d" % (n[0], n[0] % 100)
        if docid is not None and mapped and docid not in ids:
            ids.append(docid)
        if name:
            case[name] = len(docs)
        docs.append(_doc(docid, " ".join(body), docno_last))
        return docid

    def fill(k):
        return [FILL] * max(k, 0)

    def at(length, places):
        body = fill(length)
        for p, w in places.items():
            body[p] = w
        return body

    def both(text, *widths):
        for w in widths:
            queries.extend([(text, w, True), (text, w, False)])

    # -- stream lengths 0, 1, L - 1, L, L + 1, 63 .. 257 for L = 1, 2, 5, 32: the terms
    # packed and (where they fit) spread one filler apart, at the stream's start and
    # at its end
    add(["the", "of", "and", "the"], None, name="len0")
    for L in LENS:
        ph = D32[:L]
        spread = [w for t in ph for w in (t, FILL)][:-1]
        both(" ".join(ph), 1, 2, 3, MAXN)
        if L > 1:  # the width at which the packed terms just fit one window, and one below
            both(" ".join(ph), L, L - 1)
        queries += [(" ".join(ph), 2 * L - 1, False), (" ".join(ph), max(1, 2 * L - 2), False),
                    (" ".join(reversed(ph)), 2, True), (" ".join(reversed(ph)), 2 * L - 1, False)]
        for ln in sorted({L - 1, L, L + 1} | set(STREAM_LENS)):
            for terms, tag in ((ph, "p"), (spread, "s")):
                k = len(terms)
                if ln < k and tag == "p":
                    add(terms[:ln], None, name="len%d" % ln if ln < 2 else None)
                elif ln < k:
                    continue
                elif ln - k < 2:
                    add(terms + fill(ln - k), None)
                    add(fill(ln - k) + terms, None)
                else:
                    add(terms + fill(ln - k - 2), docno_last=True, name="L%d%s%d" % (L, tag, ln))  # at stream start 0
                    add(fill(ln - k - 2) + terms)  # at the stream's end
    # -- tile and carry edges (DOCNO last: body position = stream position)
    add(at(70, {62: A, 65: B}), docno_last=True, name="straddle")  # gap 3 over the tile edge
    add(at(20, {3: A, 8: B}), docno_last=True, name="gap5")  # a gap of exactly N / N + 1
    add(at(140, {1: A, 131: B}), docno_last=True, name="carry2")  # the carry over two whole tiles
    add(at(150, {10: A, 70: B, 140: Cw}), docno_last=True, name="levels")  # one level per tile
    both("%s %s" % (A, B), 2, 3, 4, 5, 6, 129, 130, 131, MAXN)
    both("%s %s %s" % (A, B, Cw), 2, 3, 69, 70, 130, 131, MAXN)
    # -- chain existence: a greedy match through the first / the last b misses these
    add([A, B, B, FILL, Cw], docno_last=True, name="greedy1")  # N = 2
    add([A, B, Cw, B], docno_last=True, name="greedy2")  # N = 3
    # -- repeated terms
    add([A, FILL, A, A], docno_last=True, name="repeat")
    both("%s %s" % (A, A), 1, 2)
    both("%s %s %s" % (A, B, A), 3, 4, MAXN)  # unordered: the set {a, b}
    # -- unordered windows: clipped at the record's start (the window of 100 ends at 1)
    add([A, B] + fill(3), docno_last=True, name="clip")
    both("%s %s" % (A, B), 100)
    # -- record boundaries: d ends with nova, d + 1 starts with oscar (words of these two only)
    add(fill(5) + ["nova"], name="end_a")
    add(["oscar"] + fill(3), docno_last=True, name="start_b")
    both("nova oscar", 1, 2, MAXN)
    dup = add([A, FILL, B], name="dup1")  # one docid in two records: freq sums
    add([A, B, FILL, A, B], dup, name="dup2")
    add([A, B, B], "MISSING7", mapped=False, name="missing")
    add([B, FILL, A], None, name="docno0")  # one more under docno 0
    # -- L = 1; unknown words; a width below |T|
    both(A, 1, 5, MAXN)
    both("%s xylophone" % A, 3)
    both("%s %s %s" % (A, B, Cw), 1)
    corpus = "".join(docs).encode("utf-8")
    return corpus, O.write_mapping(sorted(ids)), tuple(queries), case


@functools.lru_cache(maxsize=None)
def _edge_ref():
    corpus, mapping, texts, case = _edge()
    st = P.Streams(corpus, mapping)
    known = {t for _, s in st.records for t in s}
    queries = [([t if t in known else None for t in O.process_content(text)], w, o) for text, w, o in texts]
    return st, queries, case


def test_edge_corpus_is_what_it_claims():
    """(no device: the reference side of the edge corpus reaches its cases)"""
    st, queries, case = _edge_ref()
    a, b, c = (O.process_content(w)[0] for w in (A, B, Cw))
    d32 = O.process_content(" ".join(D32))
    assert len(set(d32)) == len(d32) == 32
    S = lambda name: st.records[case[name]][1]  # noqa: E731
    od, uw = NR.count_ordered, NR.count_unordered
    lens = {len(s) for _, s in st.records}
    for L in LENS:
        assert {L - 1, L, L + 1} | set(STREAM_LENS) <= lens, L
        ph = d32[:L]
        for ln in (63, 64, 65, 127, 128, 129, 257):  # packed and spread, at stream start 0 and at the end
            s = S("L%dp%d" % (L, ln))
            assert len(s) == ln and s[:L] == ph and od(s, ph, 1) == 1
            assert any(len(t) == ln and t[-L:] == ph for _, t in st.records)
            if ln >= 2 * L - 1 + 2 and L > 1:
                s = S("L%ds%d" % (L, ln))
                assert len(s) == ln and s[:2 * L - 1:2] == ph and od(s, ph, 2) == 1 and od(s, ph, 1) == 0
                assert uw(s, ph, 2 * L - 1) == 1 and uw(s, ph, 2 * L - 2) == 0
                assert any(len(t) == ln and t[-(2 * L - 1)::2] == ph for _, t in st.records)
    assert S("len0") == [] and len(S("len1")) == 1
    s = S("straddle")
    assert (s[62], s[65]) == (a, b) and od(s, [a, b], 3) == 1 and od(s, [a, b], 2) == 0
    assert uw(s, [a, b], 4) == 1 and uw(s, [a, b], 3) == 0
    s = S("gap5")
    assert od(s, [a, b], 5) == 1 and od(s, [a, b], 4) == 0
    s = S("carry2")
    assert (s[1], s[131]) == (a, b) and od(s, [a, b], 130) == 1 and od(s, [a, b], 129) == 0
    s = S("levels")
    assert (s[10], s[70], s[140]) == (a, b, c) and od(s, [a, b, c], 70) == 1 and od(s, [a, b, c], 69) == 0
    assert uw(s, [a, b, c], 131) == 1 and uw(s, [a, b, c], 130) == 0
    assert od(S("greedy1"), [a, b, c], 2) == 1 and od(S("greedy2"), [a, b, c], 3) == 1
    assert od(S("repeat"), [a, a], 2) == 2 and od(S("repeat"), [a, a], 1) == 1
    assert uw(S("clip"), [a, b], 100) == 1 and S("clip")[:2] == [a, b]
    # the record boundary: adjacent in docno order, the join would match, the records do not
    ra, rb = st.records[case["end_a"]], st.records[case["start_b"]]
    no = O.process_content("nova oscar")
    assert rb[0] == ra[0] + 1 and ra[1][-1] == no[0] and rb[1][0] == no[1]
    assert od(ra[1] + rb[1], no, 1) == 1 and uw(ra[1] + rb[1], no, 2) == 1
    for w in (1, 2, MAXN):
        assert not NR.match(st, no, w, True) and not NR.match(st, no, w, False)
    assert st.records[case["dup1"]][0] == st.records[case["dup2"]][0] > 0
    assert NR.match(st, [a, b], 2, True)[st.records[case["dup1"]][0]] == 3
    docnos = [d for d, _ in st.records]
    assert docnos.count(0) > 10 and st.records[case["missing"]][0] < 0 and st.records[case["docno0"]][0] == 0
    assert NR.match(st, [a, b], 2, True)[st.records[case["missing"]][0]] == 2
    assert NR.match(st, [a, b], 3, False)[0] >= 1
    # the query list: L = 1 and 32, the largest width, an unknown word, N < |T|
    assert {len(q[0]) for q in queries} >= {1, 2, 3, 5, 32} and any(None in q[0] for q in queries)
    assert any(q[1] == MAXN and q[2] for q in queries) and any(q[1] == MAXN and not q[2] for q in queries)
    assert not NR.match(st, [a, b, c], 2, False) and NR.match(st, d32, 32, False) and not NR.match(st, d32, 31, False)
    assert (d32, 32, False) in queries and (d32, 31, False) in queries  # 32 distinct terms in one window of 32
    assert NR.match(st, d32, 1, True) and NR.match(st, d32, 2, True) != NR.match(st, d32, 1, True)


@pytest.mark.parametrize("idf_mode", [0, 1])
def test_edge_corpus(sme, idf_mode):
    corpus, mapping, _, _ = _edge()
    st, queries, _ = _edge_ref()
    ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
    assert ix.positions()[:2] == (len(st.records), sum(len(s) for _, s in st.records))
    ids = _q(ix, queries)
    for order, m in ORDERS:
        _same(ix.query_near(ids, order, m), NR.run(st, queries, order, m, idf_mode))
    cands, verified, matches = ix.near_stats()
    assert cands >= verified >= matches > 0
    # every query as a batch of its own
    whole = ix.query_near(ids)
    assert ix.near_stats()[2] == whole[0][-1]
    for i, q in enumerate(ids):
        one = ix.query_near([q])
        assert one[0].tolist() == [0, whole[0][i + 1] - whole[0][i]]
        for k in (1, 2):
            assert np.array_equal(one[k], whole[k][whole[0][i]:whole[0][i + 1]])
        assert one[3].tobytes() == whole[3][whole[0][i]:whole[0][i + 1]].tobytes()
    # unordered with a term listed twice is the set
    two = _q(ix, [([A, B, A], 3, False), ([A, B], 3, False), ([B, B, A, A], MAXN, False), ([B, A], MAXN, False)])
    got = ix.query_near(two)
    for i in (0, 2):
        lo, mid, hi = got[0][i:i + 3]
        assert hi - mid == mid - lo > 0
        for k in (1, 2, 3):
            assert got[k][lo:mid].tobytes() == got[k][mid:hi].tobytes()


# ---- 2. cross-checks against code that exists ------------------------------------
@pytest.mark.parametrize("idf_mode", [0, 1])
def test_ordered_width_1_is_query_phrase(sme, idf_mode):
    corpus, mapping, _ = TP._edge()
    _, phrases = TP._edge_ref()
    ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
    ids = TP._ids(ix, phrases)
    assert max(len(p) for p in ids) == 32
    for order, m in ORDERS:
        want = ix.query_phrase(ids, order, m)
        _same(ix.query_near([(p, 1, True) for p in ids], order, m), want)
        assert want[0][-1] > 10
    assert ix.near_stats() == ix.phrase_stats()


def test_unordered_unbounded_is_boolean_and(sme):
    corpus, mapping, phrases, st = TP._driver()  # one record per docid
    assert len({d for d, _ in st.records}) == len(st.records)
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    ids = TP._ids(ix, phrases)
    off, dn, fq, _ = ix.query_near([(p, MAXN, False) for p in ids])
    boff, bdn, _ = ix.query_boolean([[([t], False) for t in p] for p in ids])
    assert np.array_equal(off, boff) and np.array_equal(dn, bdn) and off[-1] > 1000
    assert ix.near_stats()[1] == ix.near_stats()[2] == off[-1]  # every filter survivor matches


# ---- 3. driver and chunk edges ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _driver_queries():
    qs = []
    for n in TP.DF:
        r = TP.RARE[n]
        qs += [([r, "kilo", "lima"], 2, True), (["kilo", r, "lima"], 3, True), (["kilo", "lima", r], 2, True),
               (["lima", r, "kilo"], 3, False), ([r], 1, True), ([r, "kilo", FILL, "kilo"], 4, False)]
    qs += [(["kilo", "lima"], 1, True), (["lima", "kilo"], 2, False), ([TP.RARE[63], TP.RARE[64]], MAXN, False)]
    return qs


def test_driver_and_chunk_edges(sme):
    corpus, mapping, _, st = TP._driver()
    queries = _driver_queries()
    ix = _ctx(sme, mapping, 1, 1).build(corpus)
    ids = _q(ix, queries)
    df = np.diff(ix.offsets())
    assert [int(df[ix.lookup([TP.RARE[n]])[0]]) for n in TP.DF] == list(TP.DF)
    want = {(o, m): NR.run(st, queries, o, m, 1) for o, m in ((0, 0), (1, 0), (1, 7))}
    assert want[0, 0][0][-1] > 1000 and all(np.diff(want[0, 0][0])[6 * i + 1] > 5 for i in range(len(TP.DF)))
    try:
        for chunk in (64, 256, 1024):
            ix.ctx.set_option("bool_chunk", chunk)
            for key, w in want.items():
                _same(ix.query_near(ids, *key), w)
            stats = ix.near_stats()
            assert stats[2] == want[0, 0][0][-1] and stats[0] >= stats[1] >= stats[2]
            # the rarest term drives wherever it stands in the query
            for i, n in enumerate(TP.DF):
                for j in range(5):
                    ix.query_near([ids[6 * i + j]])
                    assert ix.near_stats()[0] == n, (n, j)
    finally:
        ix.ctx.set_option("bool_chunk", 1024)


# ---- 4. plumbing -----------------------------------------------------------------
def test_device_entry_and_independent_buffers(sme):
    corpus, mapping, phrases, st = TP._driver()
    queries = _driver_queries()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    ids = _q(ix, queries)
    host = ix.query_near(ids, 1, 9)
    _same(host, NR.run(st, queries, 1, 9, 0))
    pids = TP._ids(ix, phrases)
    ph = ix.query_phrase(pids, 1, 9)
    d_off, d_dn, d_fq, d_sc, total = ix.query_near_device(ids, 1, 9)
    d_ph = ix.query_phrase_device(pids, 1, 9)  # a phrase call in between leaves the near results alone
    ix.query_boolean([[([ids[0][0][0]], False)]])
    ix.expand_wildcards(["k*"])
    assert total == host[0][-1] > 0
    off = np.zeros(len(ids) + 1, np.int64)
    dn, fq, sc = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(total, np.float64)
    for a, p in ((off, d_off), (dn, d_dn), (fq, d_fq), (sc, d_sc)):
        sme.memcpy(a.ctypes.data, p, a.nbytes)
    _same((off, dn, fq, sc), host)
    ix.query_near(ids[:3])  # and the other way round
    got = np.zeros(d_ph[4], np.int32)
    sme.memcpy(got.ctypes.data, d_ph[1], got.nbytes)
    assert np.array_equal(got, ph[1]) and len(got) > 0
    # degenerate batches
    got = ix.query_near([([], 3, True), ids[0], (ids[0][0][:1] + [-1], 2, False), ([-1], 1, True), ([], 1, False)])
    one = ix.query_near([ids[0]])
    assert got[0].tolist() == [0, 0, one[0][1], one[0][1], one[0][1], one[0][1]] and np.array_equal(got[1], one[1])
    for entry in (ix.query_near, ix.query_near_device):
        entry([], 1, 5)
        assert ix.near_stats() == (0, 0, 0)
    got = ix.query_near([])
    assert got[0].tolist() == [0] and got[1].size == got[2].size == got[3].size == 0


def test_facade(sme):
    corpus, mapping, _, st = TP._driver()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    fw = sme.IntDocVectorsForwardIndex(ix, mapping)
    r = TP.RARE[64]
    ids = _q(ix, [(["lima", r], 0, 0)])[0][0]
    assert fw.get_near("the Lima of %s" % r.upper(), 3) == (ids, 3, False)  # stop words dropped; unordered by default
    want = NR.run(st, [(["lima", r], 3, False)], 1, 10)
    assert fw.rank_near(10) == want[1].tolist() and len(want[1]) == 10
    assert fw.get_near("lima %s" % r, 3, ordered=True) == (ids, 3, True)
    assert fw.rank_near(5) == NR.run(st, [(["lima", r], 3, True)], 1, 5)[1].tolist()
    assert fw.get_near("kilo xylophone", 2)[0][1] == -1 and fw.rank_near() == []
    assert fw.get_near("the of", 2)[0] == [] and fw.rank_near() == []


def test_refusals(sme):
    corpus, mapping, _, _ = TP._driver()
    q = [([0], 1, True)]
    plain = _ctx(sme, mapping, 1, 0, positions=0).build(corpus)
    _raises(lambda: plain.query_near(q), SME_EINVAL, "positions")
    _raises(lambda: plain.query_near_device(q), SME_EINVAL, "positions")
    _raises(lambda: plain.query_near([]), SME_EINVAL, "positions")
    grams = _ctx(sme, mapping, 2, 0).build(corpus)  # the option set, but K = 2 keeps none
    _raises(lambda: grams.query_near(q), SME_EINVAL, "K")
    ctx = _ctx(sme, mapping, 1, 0, R=2)
    loaded = ctx.load_records([bytes(plain.partition_records(p)) for p in range(2)])
    _raises(lambda: loaded.query_near(q), SME_EINVAL, "positions")
    cg = sme.Context(2, 2)
    cg.set_option("positions", 1)
    out = cg.build_chargram(corpus)
    L = sme.lib()
    t, o = np.zeros(1, np.int32), np.array([0, 1], np.int64)
    w, k = np.ones(1, np.int32), np.zeros(1, np.uint8)
    ro, dn, fq, sc = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
    rc = L.sme_query_near(out._h, t.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_int64)),
                          w.ctypes.data_as(C.POINTER(C.c_int32)), k.ctypes.data_as(C.POINTER(C.c_uint8)), 1, 0, 0,
                          C.byref(ro), C.byref(dn), C.byref(fq), C.byref(sc))
    assert rc == SME_EINVAL and b"TermKGramDocIndexer" in L.sme_last_error()
    # malformed batches and limits, the query named
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    t = int(ix.lookup(["kilo"])[0])
    one = ix.query_near([([t], 1, True)])
    for entry in (ix.query_near, ix.query_near_device):
        entry([([t] * 32, 1, True), ([t] * 32, MAXN, False)])
        _raises(lambda: entry([([t], 1, True), ([t], 0, True)]), SME_EINVAL, "query 1")
        _raises(lambda: entry([([t], -1, False)]), SME_EINVAL, "query 0")
        _raises(lambda: entry(None, arrays=(np.array([t], np.int32), np.array([0, 1], np.int64),
                                            np.array([1], np.int32), np.array([2], np.uint8))), SME_EINVAL, "query 0")
        _raises(lambda: entry([([t], 1, True), ([t] * 33, 1, False)]), SME_ELIMIT, "query 1")
        _raises(lambda: entry([([t], 1, True), ([t], 1, True), ([t, ix.V], 1, True)]), SME_EINVAL, "query 2")
        _raises(lambda: entry([([-2], 1, True)]), SME_EINVAL, "query 0")
        _raises(lambda: entry([([t], 1, True)], 2, 0), SME_EINVAL, "order")
        _raises(lambda: entry([([t], 1, True)], 0, -1), SME_EINVAL, "m must")
        _raises(lambda: entry(None, arrays=(np.array([t, t], np.int32), np.array([0, 2, 1], np.int64),
                                            np.array([1, 1], np.int32), np.zeros(2, np.uint8))), SME_EINVAL)
        _raises(lambda: entry(None, arrays=(np.array([t, t], np.int32), np.array([1, 2], np.int64),
                                            np.array([1], np.int32), np.zeros(1, np.uint8))), SME_EINVAL)
    _same(ix.query_near([([t], 1, True)]), one)  # an error leaves the index usable


def test_reweight(sme):
    corpus, mapping, _, st = TP._driver()
    queries = _driver_queries()
    ix = _ctx(sme, mapping, 1, 1).build(corpus)
    ids = _q(ix, queries)
    before = ix.query_near(ids, 1, 0)
    _same(before, NR.run(st, queries, 1, 0, 1))
    ix.reweight(2 * ix.N)
    after = ix.query_near(ids, 0, 0)
    _same(after, NR.run(st, queries, 0, 0, 1, N=2 * ix.N))
    off, dn, fq, sc = after
    x = int(off[1]) - 1  # one score by hand, with the new N
    df = int(off[1] - off[0])
    assert sc[x] == (1.0 + math.log(float(fq[x]))) * math.log10(float((2 * ix.N) // df))
    assert not np.array_equal(np.sort(before[3]), np.sort(sc))
    ix.reweight(ix.N)
    _same(ix.query_near(ids, 1, 0), before)


def test_unordered_freq_past_max_tf(sme):
    """An unordered freq can pass the largest tf of the index: the score then comes
    from the continued table, the bits of (1 + ln f) * idf."""
    bodies = [[A, B, Cw] * 3, [A, FILL, B], [Cw, FILL], [FILL, B, FILL]]
    ids = ["MT%06d-%02d" % (i, i) for i in range(1, len(bodies) + 1)]
    corpus = "".join(_doc(d, " ".join(b)) for d, b in zip(ids, bodies)).encode("utf-8")
    mapping = O.write_mapping(ids)
    st = P.Streams(corpus, mapping)
    for idf_mode in (0, 1):
        ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
        assert int(ix.csr()[2].max()) == 3
        queries = [([A, B, Cw], 3, False), ([A, B, Cw], MAXN, False), ([A, B], 3, False), ([A, B, Cw], 1, True)]
        got = ix.query_near(_q(ix, queries), 1, 0)
        _same(got, NR.run(st, queries, 1, 0, idf_mode))
        assert got[2][:2].tolist() == [7, 7] and got[0].tolist()[:3] == [0, 1, 2]
        assert got[3][0] == (1.0 + math.log(7.0)) * math.log10(float(4 // 1))
        # a later, smaller bound reads the same table
        _same(ix.query_near(_q(ix, queries[2:]), 0, 0), NR.run(st, queries[2:], 0, 0, idf_mode))
