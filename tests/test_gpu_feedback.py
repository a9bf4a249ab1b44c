"""Relevance feedback on the device (sme_index_feedback_terms*): from document sets to
their terms, over the term streams a K = 1 build keeps ("positions" 1).  Every term,
freq and docs is held to feedback_ref.py (itself held to the oracle's K = 1 index by
test_feedback_ref.py) and every score to the reference's bits or to the index's own
weights.  No tolerance anywhere: ids, counts and score.view(uint64)."""
import ctypes as C
import functools

import numpy as np
import pytest

import feedback_ref as F
import oracle_lib as O
import phrase_ref as P

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6


def _ctx(sme, mapping, k=1, idf_mode=0, positions=1, R=2):
    ctx = sme.Context(k, R, idf_mode)
    ctx.load_docno_mapping(mapping)
    if positions:
        ctx.set_option("positions", 1)
    return ctx


def _same(got, want):
    assert [a.dtype for a in got] == [np.int64, np.int32, np.int32, np.int32, np.float64]
    assert np.array_equal(got[0], want[0]), np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:8]
    for c in (1, 2, 3):
        assert np.array_equal(got[c], want[c]), (c, np.nonzero(got[c] != want[c])[0][:8])
    assert np.array_equal(got[4].view(np.uint64), want[4].view(np.uint64)), np.nonzero(got[4] != want[4])[0][:8]


def _raises(call, code, word=None):
    with pytest.raises(Exception) as e:
        call()
    assert getattr(e.value, "code", None) == code, str(e.value)
    if word is not None:
        assert word in str(e.value), str(e.value)


def _ids(ix, fb):
    """{term string: term id} of every term of the reference's streams."""
    words = sorted(fb.df)
    got = ix.lookup(words).tolist()
    assert min(got) >= 0
    return dict(zip(words, got))


_BUILT = {}


def _index(sme, name, idf_mode):
    """(index, reference, ids) of a corpus, built once per idf mode."""
    key = (name, idf_mode)
    if key not in _BUILT:
        corpus, mapping = F.corpus(name)
        ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
        fb = F.reference(name)
        _BUILT[key] = (ix, fb, _ids(ix, fb))
    return _BUILT[key]


def _check(ix, fb, ids, sets, idf_mode, **kw):
    got = ix.feedback_terms(sets, **kw)
    want, (positions, pairs, kept, missing) = fb.run(sets, ids, idf_mode=idf_mode, **kw)
    _same(got, want)
    stats = ix.feedback_stats()
    assert stats[:4] == (positions, pairs, kept, missing), (stats, (positions, pairs, kept, missing))
    return got, stats


# ---- 1. reference parity -------------------------------------------------------
@pytest.mark.parametrize("idf_mode", [0, 1])
@pytest.mark.parametrize("name", F.NAMES)
def test_reference_parity(sme, name, idf_mode):
    ix, fb, ids = _index(sme, name, idf_mode)
    sets = F.standard_sets(fb)
    got, stats = _check(ix, fb, ids, sets, idf_mode)
    assert got[0][-1] > 100 and stats[3] > 0
    got, stats = _check(ix, fb, ids, sets, idf_mode, m=0, min_df=0)
    assert stats[1] == stats[2] == got[0][-1] > 500  # nothing filtered, nothing cut
    # every set as a batch of its own gives its slice of the batch
    for i in (0, 9, 12, 13, len(sets) - 2):
        one = ix.feedback_terms([sets[i]], m=0, min_df=0)
        assert one[0].tolist() == [0, got[0][i + 1] - got[0][i]]
        for c in (1, 2, 3):
            assert np.array_equal(one[c], got[c][got[0][i]:got[0][i + 1]])
        assert one[4].tobytes() == got[4][got[0][i]:got[0][i + 1]].tobytes()


# ---- 2. no formula: a singleton set gives the index's own postings and weights ---
@pytest.mark.parametrize("idf_mode", [0, 1])
def test_singletons_are_the_index_own_postings(sme, idf_mode):
    ix, fb, _ = _index(sme, "fuzz", idf_mode)
    o, d, tf, _ = ix.csr()
    woff, wdn, w = ix.weights()
    term_o = np.repeat(np.arange(ix.V, dtype=np.int32), np.diff(o))
    term_w = np.repeat(np.arange(ix.V, dtype=np.int32), np.diff(woff))
    docnos = [x for x in sorted(fb.by_docno) if fb.count([x])[0]]
    docnos = docnos[:12] + docnos[-6:]
    assert 0 in docnos and min(docnos) < 0
    off, term, freq, docs, score = ix.feedback_terms([[x] for x in docnos], m=0, min_df=0)
    for i, x in enumerate(docnos):
        sl = slice(off[i], off[i + 1])
        tfs = dict(zip(term_o[d == x].tolist(), tf[d == x].tolist()))
        ws = dict(zip(term_w[wdn == x].tolist(), w[wdn == x].view(np.uint64).tolist()))
        assert len(tfs) > 0 and set(tfs) == set(ws) == set(term[sl].tolist())
        assert dict(zip(term[sl].tolist(), freq[sl].tolist())) == tfs
        assert dict(zip(term[sl].tolist(), score[sl].view(np.uint64).tolist())) == ws
        assert np.all(docs[sl] == 1)


# ---- 3. the two paths ----------------------------------------------------------
def _with_slots(ix, slots, call):
    ix.ctx.set_option("fb_slots", slots)
    try:
        return call()
    finally:
        ix.ctx.set_option("fb_slots", 4096)


def test_small_table_spills_and_agrees(sme):
    ix, fb, ids = _index(sme, "split", 1)
    big = fb.st.records[F.BIG_RECORD][0]
    pos = [x for x in sorted(fb.by_docno) if x > 0]
    sets = [[big], pos[20:30], [pos[0]], [], pos[40:50]]
    assert len(fb.count([big])[0]) >= 100
    base = ix.feedback_terms(sets, m=0, min_df=0)
    assert ix.feedback_stats()[4] == 0
    small = _with_slots(ix, 16, lambda: (ix.feedback_terms(sets, m=0, min_df=0), ix.feedback_stats()))
    assert small[1][4] >= 3 and small[1][:4] == ix.feedback_stats()[:4]
    _same(small[0], base)
    _same(base, fb.run(sets, ids, m=0, min_df=0, idf_mode=1)[0])
    for kw in ({}, {"m": 3, "min_docs": 2}):
        _with_slots(ix, 16, lambda: _check(ix, fb, ids, sets, 1, **kw))


def test_exactly_at_the_load_limit(sme):
    """fb_slots 16 holds 12 distinct terms: a set of 12 stays on chip, one of 13 spills."""
    ix, fb, ids = _index(sme, "split", 0)
    distinct = {x: len(fb.count([x])[0]) for x in fb.by_docno if x > 0}
    at = [x for x, n in sorted(distinct.items()) if n == 12][:2]
    past = [x for x, n in sorted(distinct.items()) if n == 13][:2]
    assert len(at) == 2 and len(past) == 2
    assert [len(fb.count([x])[0]) for x in at + past] == [12, 12, 13, 13]

    def run():
        out = []
        for sets, spilled in (([[at[0]]], 0), ([[past[0]]], 1), ([[at[0]], [past[0]], [at[1]], [past[1]]], 2)):
            _, stats = _check(ix, fb, ids, sets, 0, m=0, min_df=0)
            out.append(stats[4] == spilled)
        return out
    assert _with_slots(ix, 16, run) == [True, True, True]
    # the same rule at the next size: 24 of 32
    pairs = [(a, b) for a in at for b in sorted(distinct)[:60] if a != b]
    n24 = [p for p in pairs if len(fb.count(list(p))[0]) == 24][:1]
    n25 = [p for p in pairs if len(fb.count(list(p))[0]) == 25][:1]
    assert n24 and n25

    def run32():
        _check(ix, fb, ids, [list(n24[0])], 0, m=0, min_df=0)
        a = ix.feedback_stats()[4]
        _check(ix, fb, ids, [list(n25[0])], 0, m=0, min_df=0)
        return a, ix.feedback_stats()[4]
    assert _with_slots(ix, 32, run32) == (0, 1)


LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def _lengths():
    """One record per stream length of LENGTHS.  A docid of one token heads its
    record's stream, so a record of length L has L - 1 body words; the record of
    length 0 has no DOCNO and only stop words (docno 0)."""
    docs, docids = ["<DOC>\n<TEXT>\nthe of and\n</TEXT>\n</DOC>\n"], []
    for L in LENGTHS[1:]:
        docid = "RL%04d" % L
        docids.append(docid)
        body = " ".join("q%03d" % ((j * j + 7 * j) % 211) for j in range(L - 1))
        docs.append("<DOC>\n<DOCNO>%s</DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (docid, body))
    corpus, mapping = "".join(docs).encode(), O.write_mapping(sorted(docids))
    return corpus, mapping, F.Feedback(P.Streams(corpus, mapping))


def test_record_lengths_on_both_paths(sme):
    corpus, mapping, fb = _lengths()
    assert sorted(len(s) for _, s in fb.st.records) == list(LENGTHS)
    ix = _ctx(sme, mapping, 1, 1).build(corpus)
    ids = _ids(ix, fb)
    docnos = sorted(fb.by_docno)
    sets = [[x] for x in docnos] + [docnos, docnos[::-1], docnos[3:6]]
    for slots, spilled in ((4096, False), (16, True), (64, True)):
        for kw in ({"m": 0, "min_df": 0}, {"m": 7, "min_df": 2, "min_docs": 2}):
            _, stats = _with_slots(ix, slots, lambda: _check(ix, fb, ids, sets, 1, **kw))
            assert (stats[4] > 0) == spilled and stats[0] == 3 * sum(LENGTHS) + sum(LENGTHS[3:6])


# ---- 4. the scorer table past max_tf -------------------------------------------
def test_freq_past_max_tf(sme):
    n_tf = 40
    docs, docids = [], []
    for i in range(8):
        docids.append("MT%04d" % i)
        body = " ".join(["zulu"] * n_tf) if i < 3 else " ".join(
            "w%02d %s" % ((i * 7 + j) % 23, "zulu" if i == 3 else "yank") for j in range(9))
        docs.append("<DOC>\n<DOCNO>%s</DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (docids[-1], body))
    corpus, mapping = "".join(docs).encode(), O.write_mapping(docids)
    fb = F.Feedback(P.Streams(corpus, mapping))
    max_tf = max(s.count(t) for _, s in fb.st.records for t in set(s))
    assert max_tf == n_tf
    for idf_mode in (0, 1):
        ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
        ids = _ids(ix, fb)
        three = sorted(fb.by_docno)[:3]
        got, _ = _check(ix, fb, ids, [three, three + sorted(fb.by_docno)[3:]], idf_mode, m=0, min_df=2)
        z = ids["zulu"]
        assert got[2][got[1] == z].tolist() == [3 * max_tf, 3 * max_tf + 9]
        assert got[3][got[1] == z].tolist() == [3, 4]
        assert fb.idf("zulu", idf_mode) > 0


# ---- 5. filters and cut --------------------------------------------------------
def test_filters_and_cut(sme):
    ix, fb, ids = _index(sme, "fuzz", 0)  # SME_IDF_REFERENCE: every idf is equal, scores tie by freq
    pos = [x for x in sorted(fb.by_docno) if x > 0]
    sets = [pos[:10], pos[10:14], pos[30:31], [0] + pos[50:52]]
    name = {v: k for k, v in ids.items()}
    all_, _ = _check(ix, fb, ids, sets, 0, m=0, min_df=0)
    first = all_[1][:all_[0][1]]
    # min_docs
    got, _ = _check(ix, fb, ids, sets, 0, m=0, min_df=0, min_docs=2)
    assert 0 < got[0][-1] < all_[0][-1] and got[3].min() == 2
    # df bounds cut at exactly df == bound
    dfs = sorted({fb.df[name[t]] for t in first.tolist()})
    b = dfs[len(dfs) // 2]
    assert b > 2
    for kw, inside in (({"min_df": b}, True), ({"min_df": b + 1}, False), ({"max_df": b, "min_df": 0}, True),
                       ({"max_df": b - 1, "min_df": 0}, False)):
        got, _ = _check(ix, fb, ids, sets, 0, m=0, **kw)
        kept_dfs = {fb.df[name[t]] for t in got[1][:got[0][1]].tolist()}
        assert (b in kept_dfs) == inside and kept_dfs
    # exclusion lists: -1, a term absent from the set, the set's best terms
    absent = next(t for t in range(ix.V) if t not in set(all_[1].tolist()))
    ex = [[-1, int(first[0]), absent, int(first[3])], [], [-1], [int(t) for t in all_[1][all_[0][3]:all_[0][4]][:5]]]
    got, _ = _check(ix, fb, ids, sets, 0, m=0, min_df=0, exclude=ex)
    assert got[0][-1] == all_[0][-1] - 2 - 5 and int(first[0]) not in got[1][:got[0][1]].tolist()
    x_ids, x_off = sme.Index.phrase_arrays(ex)
    _same(ix.feedback_terms(sets, m=0, min_df=0, exclude=(x_ids, x_off)), got)
    # the cut; ties at the cut resolve by term id ascending
    for m in (1, 5, 0):
        got, stats = _check(ix, fb, ids, sets, 0, m=m)
        assert stats[2] >= got[0][-1] and (m == 0 or np.all(np.diff(got[0]) <= m))
    off, term, freq, docs, score = ix.feedback_terms(sets, m=0)
    ties = 0
    for i in range(len(sets)):
        sc, tm = score[off[i]:off[i + 1]], term[off[i]:off[i + 1]]
        assert np.all(np.diff(sc) <= 0)
        eq = np.nonzero(np.diff(sc) == 0)[0]
        assert np.all(np.diff(tm)[eq] > 0)
        ties += len(eq)
        cut = ix.feedback_terms([sets[i]], m=5)
        assert cut[1].tolist() == tm[:5].tolist()
    assert ties > 20 and score[off[1] + 4] == score[off[1] + 5]  # a tie across the cut at m = 5


# ---- 6. errors -----------------------------------------------------------------
def test_refusals(sme):
    corpus, mapping = F.corpus("split")
    ix, fb, ids = _index(sme, "split", 0)
    plain = _ctx(sme, mapping, 1, 0, positions=0).build(corpus)
    _raises(lambda: plain.feedback_terms([[1]]), SME_EINVAL, "positions")
    _raises(lambda: plain.feedback_terms([]), SME_EINVAL, "positions")
    grams = _ctx(sme, mapping, 2, 0).build(corpus)
    _raises(lambda: grams.feedback_terms([[1]]), SME_EINVAL, "K")
    loaded = _ctx(sme, mapping, 1, 0).load_records([bytes(plain.partition_records(p)) for p in range(2)])
    _raises(lambda: loaded.feedback_terms([[1]]), SME_EINVAL, "positions")
    cg = sme.Context(2, 2)
    cg.set_option("positions", 1)
    out = cg.build_chargram(corpus)
    L = sme.lib()
    dn, fo = np.ones(1, np.int32), np.array([0, 1], np.int64)
    ptrs = [C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
            C.POINTER(C.c_double)()]
    rc = L.sme_index_feedback_terms(out._h, dn.ctypes.data_as(C.POINTER(C.c_int32)),
                                    fo.ctypes.data_as(C.POINTER(C.c_int64)), 1, None, None, 20, 1, 2, 0,
                                    *[C.byref(p) for p in ptrs])
    assert rc == SME_EINVAL and b"TermKGramDocIndexer" in L.sme_last_error()
    # limits and malformed batches
    ix.feedback_terms([[1] * 1024])
    _raises(lambda: ix.feedback_terms([[1], [1] * 1025]), SME_ELIMIT, "set 1")
    _raises(lambda: ix.feedback_terms(None, arrays=(np.ones(2, np.int32), np.array([0, 2, 1], np.int64))),
            SME_EINVAL, "set 1")
    _raises(lambda: ix.feedback_terms(None, arrays=(np.ones(2, np.int32), np.array([1, 2], np.int64))), SME_EINVAL)
    for kw in ({"m": -1}, {"min_docs": -1}, {"min_df": -1}, {"max_df": -1}):
        _raises(lambda: ix.feedback_terms([[1]], **kw), SME_EINVAL, list(kw)[0])
    _raises(lambda: ix.feedback_terms([[1], [2]], exclude=[[0], [ix.V]]), SME_EINVAL, "set 1")
    _raises(lambda: ix.feedback_terms([[1]], exclude=[[-2]]), SME_EINVAL, "set 0")
    ix.feedback_terms([[1]], exclude=[[ix.V - 1, -1]])
    for bad in (8, 8192, 48, 0):
        _raises(lambda: ix.ctx.set_option("fb_slots", bad), SME_EINVAL)
    # nq == 0 is valid; an error leaves the index usable
    got = ix.feedback_terms([])
    assert got[0].tolist() == [0] and all(a.size == 0 for a in got[1:]) and ix.feedback_stats() == (0, 0, 0, 0, 0)
    assert ix.feedback_terms_device(0, np.zeros(1, np.int64))[5] == 0
    _check(ix, fb, ids, [[1, 2, 3]], 0)


# ---- 7. the device entry -------------------------------------------------------
class _Dev:
    def __init__(self, sme):
        self.sme, self.L, self.bufs = sme, sme.lib(), []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.sme_device_alloc(0, max(nbytes, 16), C.byref(p)) == 0
        self.bufs.append(p)
        return p.value

    def put(self, arr):
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            self.sme.memcpy(p, arr.ctypes.data, arr.nbytes)
        return p

    def free(self):
        for p in self.bufs:
            self.L.sme_device_free(p)


def test_device_entry_takes_topk_output(sme):
    ix, fb, ids = _index(sme, "fuzz", 1)
    df = np.diff(ix.offsets())
    rare = [int(t) for t in np.nonzero(df == 2)[0][:3]]
    common = [int(t) for t in np.argsort(-df, kind="stable")[:4]]
    terms = np.array(common[:2] + rare[:1] + [-1] + common[2:] + rare[1:], np.int32)
    qoff = np.array([0, 2, 3, 4, 6, 8], np.int64)  # query 2 holds only an unknown term: a row of pads
    nq, k = len(qoff) - 1, 10
    phrase = ix.query_phrase([[common[0]]], 1, 5)
    boolean = ix.query_boolean([[([common[0]], False), ([common[1]], False)]], 1, 5)
    dev = _Dev(sme)
    try:
        d_dn, d_sc = dev.alloc(4 * nq * k), dev.alloc(8 * nq * k)
        ix.query_topk_device(dev.put(terms), dev.put(qoff), nq, k, d_dn, d_sc)
        foff = np.arange(nq + 1, dtype=np.int64) * k
        ex = (terms, qoff)
        d_off, d_term, d_freq, d_docs, d_score, total = ix.feedback_terms_device(d_dn, foff, m=8, exclude=ex)
        host_dn = np.zeros(nq * k, np.int32)
        sme.memcpy(host_dn.ctypes.data, d_dn, host_dn.nbytes)
        got = [np.zeros(nq + 1, np.int64)] + [np.zeros(total, t) for t in (np.int32, np.int32, np.int32, np.float64)]
        for a, p in zip(got, (d_off, d_term, d_freq, d_docs, d_score)):
            sme.memcpy(a.ctypes.data, p, a.nbytes)
    finally:
        dev.free()
    rows = host_dn.reshape(nq, k)
    assert np.all(rows[2] == -1) and (rows[1] == -1).sum() == k - 2 and not np.any(rows[0] == -1)
    assert total == got[0][-1] > 0 and got[0][3] == got[0][2]  # the row of pads has no terms
    want = ix.feedback_terms(None, m=8, exclude=ex, arrays=(host_dn, foff))
    _same(got, want)
    import torch
    tensor = torch.from_numpy(host_dn).to("cuda")  # a device tensor in place of the pointer
    again = ix.feedback_terms_device(tensor, foff, m=8, exclude=ex)
    term = np.zeros(total, np.int32)
    sme.memcpy(term.ctypes.data, again[1], term.nbytes)
    assert again[5] == total and np.array_equal(term, want[1])
    _same(want, fb.run([r.tolist() for r in rows], ids, m=8, idf_mode=1,
                       exclude=[terms[qoff[i]:qoff[i + 1]].tolist() for i in range(nq)])[0])
    # the host entry's arrays live until the next feedback call, whatever else is called
    L = sme.lib()
    ptrs = [C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
            C.POINTER(C.c_double)()]
    plain = ix.feedback_terms(None, m=8, arrays=(host_dn, foff))  # (copied at once)
    assert L.sme_index_feedback_terms(ix._h, host_dn.ctypes.data_as(C.POINTER(C.c_int32)),
                                      foff.ctypes.data_as(C.POINTER(C.c_int64)), nq, None, None, 8, 1, 2, 0,
                                      *[C.byref(p) for p in ptrs]) == 0
    phrase2 = ix.query_phrase([[common[0]]], 1, 5)
    boolean2 = ix.query_boolean([[([common[0]], False), ([common[1]], False)]], 1, 5)
    ix.query_near([([common[0], common[1]], 5, False)])
    n = int(plain[0][-1])
    assert np.array_equal(np.ctypeslib.as_array(ptrs[0], (nq + 1,)), plain[0])
    assert np.array_equal(np.ctypeslib.as_array(ptrs[1], (n,)), plain[1])
    assert np.array_equal(np.ctypeslib.as_array(ptrs[3], (n,)), plain[3])
    assert np.ctypeslib.as_array(ptrs[4], (n,)).tobytes() == plain[4].tobytes()
    # a phrase and a Boolean result taken before the feedback calls are what they were
    for a, b in zip(phrase + boolean, phrase2 + boolean2):
        assert a.tobytes() == b.tobytes() and len(a) > 0


def test_other_results_survive_a_feedback_call(sme):
    ix, fb, ids = _index(sme, "fuzz", 1)
    df = np.diff(ix.offsets())
    a, b = [int(t) for t in np.argsort(-df, kind="stable")[:2]]
    d_ph = ix.query_phrase_device([[a]], 1, 6)
    d_bq = ix.query_boolean_device([[([a], False), ([b], False)]], 1, 6)
    want_ph, want_bq = ix.query_phrase([[a]], 1, 6), ix.query_boolean([[([a], False), ([b], False)]], 1, 6)
    d_ph = ix.query_phrase_device([[a]], 1, 6)
    d_bq = ix.query_boolean_device([[([a], False), ([b], False)]], 1, 6)
    ix.feedback_terms(F.standard_sets(fb), m=0, min_df=0)
    got = np.zeros(d_ph[4], np.int32)
    sme.memcpy(got.ctypes.data, d_ph[1], got.nbytes)
    assert np.array_equal(got, want_ph[1]) and len(got) == 6
    got = np.zeros(d_bq[3], np.int32)
    sme.memcpy(got.ctypes.data, d_bq[1], got.nbytes)
    assert np.array_equal(got, want_bq[1]) and len(got) == 6


# ---- 8. the facade -------------------------------------------------------------
def test_facade(sme):
    corpus, mapping = F.corpus("c1")
    ix, fb, ids = _index(sme, "c1", 1)
    fw = sme.IntDocVectorsForwardIndex(ix, mapping)
    pos = [x for x in sorted(fb.by_docno) if x > 0 and len(fb.count([x])[0]) > 30]
    for docno in pos[:3]:
        sim = fw.get_similar(docno, terms=25)
        want = fb.run([[docno]], ids, m=25, idf_mode=1)[0]
        assert sim == want[1].tolist() and len(sim) == 25
        ranked = fw.rank_similar(10)
        dn, _ = ix.query_topk(np.array(sim, np.int32), np.array([0, len(sim)], np.int64), 11)
        assert docno in dn[0].tolist()  # the document is most like itself: removing it matters
        assert ranked == [int(x) for x in dn[0] if x >= 0 and x != docno][:10] and docno not in ranked
        assert len(ranked) == 10
    assert fw.get_similar(max(fb.by_docno) + 9) == [] and fw.rank_similar() == []
    # query_feedback is the four steps by hand
    df = np.diff(ix.offsets())
    mid = [int(t) for t in np.nonzero((df >= 5) & (df <= 40))[0][:12]]
    terms = np.array(mid + [-1], np.int32)
    qoff = np.array([0, 2, 5, 6, 12, 12, 13], np.int64)  # an empty query and one of only -1 among them
    nq = len(qoff) - 1
    dn1, _ = ix.query_topk(terms, qoff, 7)
    exp = ix.feedback_terms([r.tolist() for r in dn1], m=9,
                            exclude=[terms[qoff[i]:qoff[i + 1]].tolist() for i in range(nq)])
    parts, xoff = [], [0]
    for i in range(nq):
        parts += terms[qoff[i]:qoff[i + 1]].tolist() + exp[1][exp[0][i]:exp[0][i + 1]].tolist()
        xoff.append(len(parts))
    want_dn, want_sc = ix.query_topk(np.array(parts, np.int32), np.array(xoff, np.int64), 10)
    dn, sc, xt, xo = ix.query_feedback(terms, qoff, k=10, fb_docs=7, fb_terms=9)
    assert xt.tolist() == parts and xo.tolist() == xoff and exp[0][-1] > 20
    assert np.array_equal(dn, want_dn) and sc.tobytes() == want_sc.tobytes()
    assert not np.array_equal(dn, ix.query_topk(terms, qoff, 10)[0])  # the expansion changes the ranking
    # fb_terms = 0: plain query_topk
    dn, sc, xt, xo = ix.query_feedback(terms, qoff, k=10, fb_docs=7, fb_terms=0)
    base = ix.query_topk(terms, qoff, 10)
    assert np.array_equal(dn, base[0]) and sc.tobytes() == base[1].tobytes() and xt.tolist() == terms.tolist()
    # rank_feedback: one query through query_feedback
    word = next(w for w in (ix.term(t) for t in mid) if min(ix.lookup(ix.ctx.process_content(w)), default=-1) >= 0)
    got = fw.rank_feedback(word, k=10, fb_docs=5, fb_terms=6)
    t = ix.lookup(ix.ctx.process_content(word))
    t = np.array([int(x) for x in t if x >= 0], np.int32)
    want = ix.query_feedback(t, np.array([0, len(t)], np.int64), 10, 5, 6)[0]
    assert len(t) > 0 and got == [int(x) for x in want[0] if x >= 0] and len(got) > 0
