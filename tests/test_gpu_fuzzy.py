"""Spelling suggestions on the device (sme_index_suggest_terms*): every result is
held to the dynamic-programming restatement of fuzzy_ref.py applied to the
index's terms and posting counts -- offsets, term ids and distances exactly
equal, which includes the order (distance asc, df desc, term id asc) and the
cut -- over vocabularies loaded from hand-written record streams (term i with
1 + (7 i) % 5 postings, so df varies) and one built index."""
import functools
import random

import numpy as np
import pytest

import common
import fuzzy_ref as F
import load_streams as S
import wild_ref as W

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
NDOCS = 8


def _load(sme, terms, R=1):
    """An index whose vocabulary is exactly `terms` (String.compareTo order), term
    i with F.df_of(i) postings, the doc counter in a partition of its own."""
    assert terms == sorted(terms, key=W.unit_key) and len(set(terms)) == len(terms)
    body = b"".join(S.record(W.mutf8(t), [(d, 1) for d in range(1, 1 + F.df_of(i))]) for i, t in enumerate(terms))
    ix = sme.Context(1, R).load_records([body, S.counter(S.counter_posts(list(range(1, NDOCS + 1))))])
    assert ix.V == len(terms)
    return ix


class Ref:
    """The restatement over one vocabulary; distances are computed once per word."""

    def __init__(self, terms, df):
        self.terms, self.df, self.vocab, self.cache = terms, np.asarray(df), F.Vocab(terms), {}

    def suggest(self, words, max_dist, m):
        return F.suggest(words, self.vocab, self.df, max_dist, m, self.cache)

    def nearest(self, word):
        self.suggest([word], 0, 0)
        return int(self.cache[word].min())


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.uint8
    assert np.array_equal(got[0], want[0]), np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:5]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])


def _check(ix, ref, words, max_dist, m):
    got = ix.suggest_terms(words, max_dist, m)
    _same(got, ref.suggest(words, max_dist, m))
    return got


@pytest.fixture(scope="module")
def small(sme):
    terms = W.small_terms()
    ix = _load(sme, terms)
    assert ix.terms() == terms
    df = ix.csr()[3]
    assert df.tolist() == [F.df_of(i) for i in range(len(terms))]
    return ix, Ref(terms, df)


@functools.lru_cache(maxsize=None)
def _big_ref():
    terms = W.big_terms()
    return Ref(terms, [F.df_of(i) for i in range(len(terms))])


@pytest.fixture(scope="module")
def big(sme):
    ref = _big_ref()
    ix = _load(sme, ref.terms)
    assert ix.term(0) == ref.terms[0] and ix.term(ix.V - 1) == ref.terms[-1] and ix.term(12345) == ref.terms[12345]
    return ix, ref


@functools.lru_cache(maxsize=None)
def _fuzz():
    return common.fuzz_corpus(8, 120)


@pytest.fixture(scope="module")
def built(sme):
    corpus, ids = _fuzz()
    ctx = sme.Context(1, 3)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    ix = ctx.build(corpus)
    return ix, Ref(ix.terms(), ix.csr()[3])


def _one_edit_words(terms, n, seed):
    """n terms of 5..40 units with one seeded edit each."""
    rng = random.Random(seed)
    pool = [t for t in terms if 5 <= len(W.units(t)) <= 40]
    return [F.random_edit(rng, t, "abcdefghijklmnopqrstuvwxyz") for t in rng.sample(pool, n)]


@pytest.mark.parametrize("max_dist", [0, 1, 2, 3])
def test_word_set(small, max_dist):
    ix, ref = small
    terms = ref.terms
    # the set reaches what it is meant to reach
    for k, w in F.FAR.items():
        assert ref.nearest(w) == k
    assert F.FAR[max_dist + 1] in F.WORDS
    assert all(F.needs_scan(w, 1) for w in ("a", "ab", "abc", "")) and F.needs_scan("", 0)
    assert sum(not F.needs_scan(w, max_dist) for w in F.WORDS) >= 5 and sum(F.needs_scan(w, max_dist) for w in F.WORDS)
    for m in (0, 1, 3):
        off, ids, dist = _check(ix, ref, F.WORDS, max_dist, m)
        got = {w: (ids[off[i]:off[i + 1]].tolist(), dist[off[i]:off[i + 1]].tolist()) for i, w in enumerate(F.WORDS)}
        assert got[F.FAR[max_dist + 1]] == ([], [])
        assert got["apple"][0][0] == terms.index("apple") and got["apple"][1][0] == 0
        assert got["a" * 64] == ([], []) and got["a*c"][1][:1] != [0] and got["a?c"][1][:1] != [0]
        if max_dist >= 1:
            assert terms.index(W.AS) in ix.suggest_terms(["a" * 61], max_dist, 0)[1]
            assert got["apply"][0][0] == terms.index("apply") and terms.index("apple") in \
                ix.suggest_terms(["apply"], max_dist, 0)[1]
            assert got["\ud83d"][1][0] == 1
        if m == 0:
            # "appel" is two edits from "apple" (no transposition); the empty word reaches the short terms
            assert (terms.index("apple") in got["appel"][0]) == (max_dist >= 2)
            assert got[""][0] == [t for t, _ in F.ranked(ref.vocab.len, ref.df, max_dist)]
            assert (terms.index(W.SUPP + "smile") in got[W.SUPP + "smil"][0]) == (max_dist >= 1)
        # each word as a batch of its own
        for i, w in enumerate(F.WORDS):
            o1, i1, d1 = ix.suggest_terms([w], max_dist, m)
            assert o1.tolist() == [0, len(got[w][0])] and (i1.tolist(), d1.tolist()) == got[w], w
    if max_dist == 0:
        off, ids, dist = ix.suggest_terms(F.WORDS, 0, 0)
        look = ix.lookup(F.WORDS)
        for i, w in enumerate(F.WORDS):
            assert ids[off[i]:off[i + 1]].tolist() == ([int(look[i])] if look[i] >= 0 else []), w
        assert not dist.any() and (look >= 0).sum() >= 8 and (look < 0).sum() >= 8


def test_ordering(small):
    ix, ref = small
    want = F.ranked(ref.vocab.distances("a"), ref.df, 1)
    at1 = [int(ref.df[t]) for t, d in want if d == 1]
    assert len(set(at1)) >= 3 and max(at1.count(x) for x in set(at1)) >= 2  # the case is there
    off, ids, dist = _check(ix, ref, ["a"], 1, 0)
    key = [(int(d), -int(ref.df[t]), int(t)) for t, d in zip(ids, dist)]
    assert key == sorted(key) and len(key) == len(want) and dist[0] == 0
    o1, i1, d1 = ix.suggest_terms(["a", "zzq"], 1, 1)
    assert o1.tolist() == [0, 1, 2] and i1[0] == ids[0] and ref.terms[i1[1]] == "zz" and d1.tolist() == [0, 1]
    o2, i2, d2 = _check(ix, ref, ["a", "b", "a"], 1, 4)
    assert i2[:4].tolist() == ids[:4].tolist() and i2[8:].tolist() == ids[:4].tolist()


def test_boundaries_cannot_alias(sme):
    terms = W.BOUNDARY_TERMS
    ix = _load(sme, terms)
    assert ix.terms() == terms
    ref = Ref(terms, [F.df_of(i) for i in range(len(terms))])
    off, ids, dist = _check(ix, ref, F.BOUNDARY_WORDS, 1, 0)
    got = {w: {terms[t]: int(d) for t, d in zip(ids[off[i]:off[i + 1]], dist[off[i]:off[i + 1]])}
           for i, w in enumerate(F.BOUNDARY_WORDS)}
    # a literal '$', U+0000 or U+FFFF is one more unit, never START / END
    assert got["ab"]["ab"] == 0 and got["ab"]["$ab"] == 1 and got["ab"]["\u0000ab"] == 1 and got["ab"]["ab\uffff"] == 1
    assert got["$ab"]["$ab"] == 0 and got["$ab"]["ab"] == 1 and got["ab\uffff"]["ab\uffff"] == 0
    assert "ab$" not in got["$ab"] and "$ab" not in got["ab\uffff"]
    for d in (0, 2):
        _check(ix, ref, F.BOUNDARY_WORDS, d, 0)


def test_big_vocabulary_sources_and_chunks(big):
    ix, ref = big
    V = len(ref.terms)
    words = F.big_words(ref.terms)
    assert len(words) == 48
    # by construction no word falls back to the scan, and the chosen lists are short
    assert sum(F.needs_scan(w, 2) for w in words) == 0
    tab = W.table(ref.terms)
    lists = [F.chosen_lists(w, tab, 2) for w in words]
    assert all(len(ls) == 7 for ls in lists)
    assert sum(len(set().union(*map(set, ls))) for ls in lists) < 48 * V // 4
    assert sum(sum(map(len, ls)) for ls in lists) < 48 * V // 4
    want = ref.suggest(words, 2, 0)
    assert want[0][-1] >= 30 and int(np.sum(want[2] > 0)) >= 20
    outs, stats = [], {}
    try:
        for scan in (0, 1):
            ix.ctx.set_option("fuzzy_scan", scan)
            for chunk in (64, 1024):
                ix.ctx.set_option("wild_chunk", chunk)
                outs.append(ix.suggest_terms(words, 2, 0))
                stats[scan, chunk] = ix.suggest_stats()
    finally:
        ix.ctx.set_option("fuzzy_scan", 0)
        ix.ctx.set_option("wild_chunk", 1024)
    for got in outs:
        _same(got, want)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, outs[0]))
    for chunk in (64, 1024):
        assert stats[0, chunk][0] == 0 and stats[0, chunk][1] < 48 * V // 4
        assert stats[0, chunk][1] == sum(sum(map(len, ls)) for ls in lists)
        assert stats[1, chunk] == (48, 48 * V)
    # words that do scan, beside words that do not, in one batch
    mixed = words[:6] + ["ab", "", "abc9"] + words[6:12]
    _check(ix, ref, mixed, 2, 5)
    assert ix.suggest_stats()[0] == 3


def test_built_index(built):
    ix, ref = built
    words = _one_edit_words(ref.terms, 40, 4)
    for max_dist, m in ((1, 0), (2, 10), (3, 2)):
        off, ids, dist = _check(ix, ref, words, max_dist, m)
        assert int(np.sum(np.diff(off) > 0)) >= 36
    ix.ctx.set_option("fuzzy_scan", 1)
    try:
        _check(ix, ref, words, 2, 10)
    finally:
        ix.ctx.set_option("fuzzy_scan", 0)


def _stable_pair(ix, ref):
    """(term T, misspelling M): both pass processContent unchanged, M is unknown
    and its best suggestion is T at one edit."""
    rng = random.Random(2)
    pool = [t for t in ref.terms if 7 <= len(t) <= 10 and t.isascii() and t.isalpha()]
    for t in rng.sample(pool, len(pool)):
        p = len(t) // 2
        m = t[:p] + ("q" if t[p] != "q" else "x") + t[p + 1:]
        if ix.ctx.process_content(t) != [t] or ix.ctx.process_content(m) != [m] or ix.lookup([m])[0] >= 0:
            continue
        o, i, d = ref.suggest([m], 2, 1)
        if i.tolist() == [ref.terms.index(t)] and d.tolist() == [1]:
            return t, m
    raise AssertionError("no stable pair in the corpus")


def test_device_entry_and_splice(sme, built):
    import torch
    ix, ref = built
    words = _one_edit_words(ref.terms, 40, 4)
    for batch, max_dist, m in ((words, 2, 3), (["zzzzzzzzzzzzzzzzqq"], 1, 0), ([], 2, 10)):
        off, ids, dist = ix.suggest_terms(batch, max_dist, m)
        d_off, d_ids, d_dist, total = ix.suggest_terms_device(batch, max_dist, m)
        assert total == off[-1] and d_off
        got_off = np.zeros(len(batch) + 1, np.int64)
        sme.memcpy(got_off.ctypes.data, d_off, got_off.nbytes)
        got_ids, got_dist = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.uint8)
        if total:
            sme.memcpy(got_ids.ctypes.data, d_ids, 4 * total)
            sme.memcpy(got_dist.ctypes.data, d_dist, total)
        assert np.array_equal(got_off, off) and np.array_equal(got_ids[:total], ids)
        assert np.array_equal(got_dist[:total], dist)
    # a misspelt word's best suggestion spliced into a device query batch
    t, m = _stable_pair(ix, ref)
    tid, other = ref.terms.index(t), int(ix.lookup(ix.ctx.process_content("running"))[0])
    assert other >= 0
    k = 10
    st = torch.cuda.current_stream().cuda_stream
    q_ok = torch.tensor([tid, other], dtype=torch.int32, device="cuda")
    q_fix = torch.tensor([-1, other], dtype=torch.int32, device="cuda")
    qoff = torch.tensor([0, 2], dtype=torch.int64, device="cuda")
    out = [(torch.empty((1, k), dtype=torch.int32, device="cuda"), torch.empty((1, k), dtype=torch.float64, device="cuda"))
           for _ in range(2)]
    torch.cuda.synchronize()
    d_off, d_ids, d_dist, total = ix.suggest_terms_device(["nosuchwordatall", m], 2, 1, st)
    assert total == 1
    got_off = np.zeros(3, np.int64)
    sme.memcpy(got_off.ctypes.data, d_off, got_off.nbytes)
    assert got_off.tolist() == [0, 0, 1]
    sme.memcpy(q_fix.data_ptr(), d_ids + 4 * int(got_off[1]), 4, st)  # term_ids[sug_off[1]], device to device
    ix.query_topk_device(q_fix.data_ptr(), qoff.data_ptr(), 1, k, out[0][0].data_ptr(), out[0][1].data_ptr(), st)
    ix.query_topk_device(q_ok.data_ptr(), qoff.data_ptr(), 1, k, out[1][0].data_ptr(), out[1][1].data_ptr(), st)
    torch.cuda.synchronize()
    assert q_fix.cpu().tolist() == [tid, other]
    assert out[0][0].cpu().numpy().tobytes() == out[1][0].cpu().numpy().tobytes()
    assert out[0][1].cpu().numpy().tobytes() == out[1][1].cpu().numpy().tobytes()
    assert float(out[1][1][0, 0]) > 0.0  # the query has results (docnos of unmapped docids are negative)
    # the facade
    fw = sme.IntDocVectorsForwardIndex(ix)
    assert fw.get_corrected([m, "running", "nosuchwordatall"]) == [(m, t)]
    assert fw._terms == [tid, other]
    fixed = fw.rank()
    fw.getValue(ix.ctx.process_content(t + " running"))
    assert fixed == fw.rank() and fixed
    assert fw.get_corrected(["running"]) == [] and fw._terms == [other]
    assert fw.get_corrected(["nosuchwordatall"], max_dist=1) == [] and fw.rank() == []


def test_coexistence_with_wildcards(sme, built):
    ix, ref = built
    patterns = ["appl*", "*ing", "a?c", "run*"]
    words = _one_edit_words(ref.terms, 12, 9)
    w0 = ix.expand_wildcards(patterns)
    stats = ix.wildcard_stats()
    _, d_wids, wtotal = ix.expand_wildcards_device(patterns)
    s0 = _check(ix, ref, words, 2, 10)
    # the last expansion's device buffer is as it was
    ids_after = np.zeros(max(wtotal, 1), np.int32)
    sme.memcpy(ids_after.ctypes.data, d_wids, 4 * wtotal)
    assert wtotal == w0[0][-1] and np.array_equal(ids_after[:wtotal], w0[1])
    w1 = ix.expand_wildcards(patterns)
    assert w1[0].tobytes() == w0[0].tobytes() and w1[1].tobytes() == w0[1].tobytes()
    assert ix.wildcard_stats() == stats  # the table was built once
    # the other way round: an expansion leaves the last suggestions' device buffers alone
    d_off, d_ids, d_dist, total = ix.suggest_terms_device(words, 2, 10)
    ix.expand_wildcards(["*"])
    got = np.zeros(max(total, 1), np.int32)
    sme.memcpy(got.ctypes.data, d_ids, 4 * total)
    assert total == s0[0][-1] and np.array_equal(got[:total], s0[1])
    # reweight changes weights, not posting counts: the suggestions stay
    ix.reweight(2 * ix.N)
    try:
        assert np.array_equal(ix.csr()[3], ref.df)
        s1 = ix.suggest_terms(words, 2, 10)
    finally:
        ix.reweight(ix.N)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(s0, s1))
    assert ix.wildcard_stats() == stats


def test_refusals(sme, small, built):
    ix, ref = small
    ok = ["appel", "runing"]

    def intact():
        _check(ix, ref, ok, 2, 3)

    with pytest.raises(sme.SmeError) as e:
        ix.suggest_terms(["apple", F.TOO_LONG])
    assert e.value.code == SME_ELIMIT and "word 1" in str(e.value)
    intact()
    with pytest.raises(sme.SmeError) as e:
        ix.suggest_terms(["apple", "b", F.MALFORMED])
    assert e.value.code == SME_EINVAL and "word 2" in str(e.value)
    intact()
    for bad in (b"\x80", b"\xc3", b"\xf0\x9f\x98", b"\xc0\xaf"):
        with pytest.raises(sme.SmeError) as e:
            ix.suggest_terms([bad])
        assert e.value.code == SME_EINVAL
    for max_dist, m in ((4, 10), (-1, 10), (2, -1)):
        with pytest.raises(sme.SmeError) as e:
            ix.suggest_terms(ok, max_dist, m)
        assert e.value.code == SME_EINVAL
        with pytest.raises(sme.SmeError) as e:
            ix.suggest_terms_device(ok, max_dist, m)
        assert e.value.code == SME_EINVAL
        intact()
    for bad in (2, -1):
        with pytest.raises(sme.SmeError) as e:
            ix.ctx.set_option("fuzzy_scan", bad)
        assert e.value.code == SME_EINVAL
    intact()
    assert len(W.units("a" * 63 + "é")) == 64
    _check(ix, ref, ["a" * 63 + "é"], 3, 0)  # 64 units: accepted
    off, ids, dist = ix.suggest_terms([], 2, 10)
    assert off.tolist() == [0] and ids.size == 0 and dist.size == 0
    assert ix.suggest_stats() == (0, 0)
    # index kinds without a term vocabulary of their own
    bix, bref = built
    corpus, docids = _fuzz()
    cg = sme.Context(2, 2).build_chargram(corpus)
    ctx2 = sme.Context(2, 2)
    ctx2.load_docno_mapping(sme.TrecDocnoMapping.write(docids))
    k2 = ctx2.build(corpus)
    import torch
    sizes = bix.pack_pieces(1)
    blob = torch.empty(max(sum(sizes), 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bix.pack_pieces(1, blob.data_ptr())
    merged = bix.ctx.merge_pieces(blob.data_ptr(), sizes)
    for obj, word in ((cg, "CharKGramTermIndexer"), (k2, "K = 2"), (merged, "records-only")):
        for call in (lambda: sme.Index.suggest_terms(obj, ["apple"]),
                     lambda: sme.Index.suggest_terms_device(obj, ["apple"])):
            with pytest.raises(sme.SmeError) as e:
                call()
            assert e.value.code == SME_EINVAL and word in str(e.value), str(e.value)
    _check(bix, bref, ["appel"], 2, 3)
    # an index without terms answers every word with nothing
    empty = ix.ctx.load_records([])
    off0, ids0, dist0 = empty.suggest_terms(["", "a", "apple"], 3, 0)
    assert off0.tolist() == [0, 0, 0, 0] and ids0.size == 0 and dist0.size == 0
    # loaded from its own record streams, the built index suggests the same
    parts = [bytes(bix.partition_records(p)) for p in range(bix.ctx.num_partitions)]
    loaded = sme.Context(1, 3).load_records(parts)
    _check(loaded, bref, _one_edit_words(bref.terms, 10, 6), 2, 10)
