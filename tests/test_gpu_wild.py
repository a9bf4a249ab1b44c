"""Wildcard term expansion on the device (sme_index_expand_wildcards*): every
result is held to the Python `re` restatement of wild_ref.py applied to
ix.terms() -- term ids exactly equal and ascending, offsets exactly equal -- over
vocabularies loaded from hand-written record streams and one built index."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import common
import load_streams as S
import wild_ref as W

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
NDOCS = 8


def _load(sme, terms, R=1):
    """An index whose vocabulary is exactly `terms` (String.compareTo order): one
    posting per term, the doc counter in a partition of its own."""
    assert terms == sorted(terms, key=W.unit_key) and len(set(terms)) == len(terms)
    body = b"".join(S.record(W.mutf8(t), [(1 + i % NDOCS, 1)]) for i, t in enumerate(terms))
    ix = sme.Context(1, R).load_records([body, S.counter(S.counter_posts(list(range(1, NDOCS + 1))))])
    assert ix.V == len(terms)
    return ix


def _check(ix, patterns, terms=None):
    """One batch against the restatement; returns the device's arrays."""
    terms = ix.terms() if terms is None else terms
    off, ids = ix.expand_wildcards(patterns)
    want_off, want_ids = W.expand(patterns, terms)
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert np.array_equal(off, want_off), [p for i, p in enumerate(patterns)
                                           if off[i + 1] - off[i] != want_off[i + 1] - want_off[i]][:5]
    assert np.array_equal(ids, want_ids)
    for i in range(len(patterns)):
        assert np.all(np.diff(ids[off[i]:off[i + 1]]) > 0)
    return off, ids


@pytest.fixture(scope="module")
def small(sme):
    ix = _load(sme, W.small_terms())
    terms = ix.terms()
    assert terms == W.small_terms()
    return ix, terms


@functools.lru_cache(maxsize=None)
def _big_terms():
    return W.big_terms()


@pytest.fixture(scope="module")
def big(sme):
    terms = _big_terms()
    ix = _load(sme, terms)
    assert ix.term(0) == terms[0] and ix.term(ix.V - 1) == terms[-1] and ix.term(12345) == terms[12345]
    return ix, terms


@functools.lru_cache(maxsize=None)
def _fuzz():
    corpus, ids = common.fuzz_corpus(8, 120)
    return corpus, ids


@pytest.fixture(scope="module")
def built(sme):
    corpus, ids = _fuzz()
    ctx = sme.Context(1, 3)
    ctx.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    return ctx.build(corpus)


def test_pattern_set(small):
    ix, terms = small
    off, ids = _check(ix, W.PATTERNS, terms)
    got = {p: ids[off[i]:off[i + 1]].tolist() for i, p in enumerate(W.PATTERNS)}
    # the set reaches what it is meant to reach
    assert got["apple"] == [terms.index("apple")] and got["absent"] == [] and got[""] == []
    assert got["*"] == list(range(len(terms))) and got["**"] == got["*"] and got["z" * 130] == []
    assert got["a*a*a*a*b"] and terms.index(W.AS) not in got["a*a*a*a*b"] and terms.index(W.AS) in got["a*a*a*a*a"]
    assert got["?"] == [i for i, t in enumerate(terms) if len(W.units(t)) == 1]
    assert terms.index(W.SUPP) in got["??"] and terms.index(W.SUPP) not in got["?"]
    assert got["?" * 120] == [terms.index(W.LONG)] and got["a" * 254 + "*"] == []
    # each pattern as a batch of its own
    for p in W.PATTERNS:
        o1, i1 = ix.expand_wildcards([p])
        assert o1.tolist() == [0, len(got[p])] and i1.tolist() == got[p], p


def test_pattern_set_built_index(built):
    _check(built, W.PATTERNS + ["appl*", "*'*", "*.*", "*é", "long*", "dots*", "fz*", "*0", "??????-??"])


def test_refused_patterns(sme, small):
    ix, terms = small
    with pytest.raises(sme.SmeError) as e:
        ix.expand_wildcards(["a*", W.TOO_LONG])
    assert e.value.code == SME_ELIMIT
    with pytest.raises(sme.SmeError) as e:
        ix.expand_wildcards(["a*", "b*", W.MALFORMED])
    assert e.value.code == SME_EINVAL and "pattern 2" in str(e.value)
    for bad in (b"\x80", b"\xc3", b"\xe2\x82*", b"\xf0\x9f\x98", b"\xc0\xaf"):
        with pytest.raises(sme.SmeError) as e:
            ix.expand_wildcards([bad])
        assert e.value.code == SME_EINVAL
    _check(ix, ["a*"], terms)  # the index is intact


def test_boundaries_cannot_alias(sme):
    ix = _load(sme, W.BOUNDARY_TERMS)
    terms = ix.terms()
    assert terms == W.BOUNDARY_TERMS
    off, ids = _check(ix, W.BOUNDARY_PATTERNS, terms)
    got = {p: [terms[t] for t in ids[off[i]:off[i + 1]]] for i, p in enumerate(W.BOUNDARY_PATTERNS)}
    assert got["ab"] == ["ab"]
    assert sorted(got["ab*"]) == sorted(["ab", "ab$", "ab￿", "abab", "abx"])
    assert sorted(got["*ab"]) == sorted(["ab", "$ab", "\u0000ab", "abab", "xab"])
    tab = W.table(terms)
    assert ix.wildcard_stats() == (len(tab), sum(len(v) for v in tab.values()))


def test_table_statistics(small, big):
    for ix, terms in (small, big):
        tab = W.table(terms)
        assert ix.wildcard_stats() == (len(tab), sum(len(v) for v in tab.values()))
        assert ix.prepare_wildcards() >= 0.0 and ix.wildcard_stats()[0] == len(tab)  # built once, kept
    # "aaaa...a" holds "aaa" many times: one pair
    k = W.term_grams("aaaa")[1]
    assert W.term_grams(W.AS).count(k) == 58 and W.table([W.AS])[k] == [0]


EDGE_COUNTS = {"a": 1, "b": 63, "c": 64, "d": 65, "e": 128, "f": 129}


def test_chunk_and_wave_edges(sme):
    marked = ["%03dzq%s%d" % (j, m, j % 10) for m, c in EDGE_COUNTS.items() for j in range(c)]
    terms = sorted(set(W.small_terms()) | set(marked), key=W.unit_key)
    ix = _load(sme, terms)
    tab = W.table(terms)
    patterns = []
    for m, c in EDGE_COUNTS.items():
        for p in ("*zq%s*" % m, "*zq%s*5" % m, "*zq%s?" % m, "0*zq%s*" % m):
            assert W.candidates(p, tab, len(terms)) == c
            patterns.append(p)
    ix.ctx.set_option("wild_chunk", 64)
    base = _check(ix, patterns, terms)
    for i, (m, c) in enumerate(EDGE_COUNTS.items()):
        assert base[0][4 * i + 1] - base[0][4 * i] == c
    for chunk in (128, 1024, 4096):
        ix.ctx.set_option("wild_chunk", chunk)
        got = ix.expand_wildcards(patterns)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    for bad in (0, 32, 100, 4160):
        with pytest.raises(sme.SmeError) as e:
            ix.ctx.set_option("wild_chunk", bad)
        assert e.value.code == SME_EINVAL
    with pytest.raises(sme.SmeError):
        ix.ctx.set_option("wild_scan", 2)


def test_whole_vocabulary_chunks(big):
    ix, terms = big
    patterns = ["*", "*a*", "?b*", "*9", "??", "*é*é*", "q*", "*zz*", "abc*", ""]
    want = W.expand(patterns, terms)
    assert want[0][1] == len(terms) and want[0][2] > want[0][1] + 1000
    outs = []
    for scan in (0, 1):
        ix.ctx.set_option("wild_scan", scan)
        for chunk in (64, 1024, 4096):
            ix.ctx.set_option("wild_chunk", chunk)
            outs.append(ix.expand_wildcards(patterns))
    ix.ctx.set_option("wild_scan", 0)
    ix.ctx.set_option("wild_chunk", 1024)
    for off, ids in outs:
        assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1])


def test_paths_agree(small, built):
    for ix in (small[0], built):
        res = {}
        for scan in (0, 1):
            ix.ctx.set_option("wild_scan", scan)
            res[scan] = [ix.expand_wildcards(W.PATTERNS)] + [ix.expand_wildcards([p]) for p in W.PATTERNS]
        ix.ctx.set_option("wild_scan", 0)
        for a, b in zip(res[0], res[1]):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _mixed_batch(terms, n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        t = rng.choice(terms)
        r = rng.random()
        if r < 0.2:
            out.append(t[:rng.randint(1, len(t))] + "*")
        elif r < 0.4:
            out.append("*" + t[rng.randrange(len(t)):])
        elif r < 0.5:
            out.append(t)
        else:  # mostly without a match
            out.append("".join(rng.choice("abcingxyz?*") for _ in range(rng.randint(1, 8))))
    out[n // 2] = "*"
    return out


def test_batch_shapes(sme, small):
    ix, terms = small
    off, ids = ix.expand_wildcards([])
    assert off.tolist() == [0] and ids.size == 0
    _check(ix, ["ab*"], terms)
    batch = _mixed_batch([t for t in terms if t.isascii()], 1000, 3)
    off, ids = _check(ix, batch, terms)
    n_none = int(np.sum(np.diff(off) == 0))
    assert n_none > 200 and off[501] - off[500] == len(terms)
    # the same expansion again, then another: each call replaces the last one's buffers
    again = ix.expand_wildcards(batch)
    assert again[0].tobytes() == off.tobytes() and again[1].tobytes() == ids.tobytes()
    _check(ix, ["*ing", "zz"], terms)
    # an index without terms answers every pattern with nothing
    empty = ix.ctx.load_records([])
    off0, ids0 = empty.expand_wildcards(["*", "a*", "abc", ""])
    assert off0.tolist() == [0, 0, 0, 0, 0] and ids0.size == 0
    assert empty.wildcard_stats() == (0, 0)


def test_reweight_and_prepare_queries_keep_the_table(built):
    ix = built
    patterns = ["appl*", "*ing", "*", "a?c", "run*"]
    before = _check(ix, patterns)
    stats = ix.wildcard_stats()
    ix.reweight(2 * ix.N)
    mid = ix.expand_wildcards(patterns)
    ix.prepare_queries()
    after = ix.expand_wildcards(patterns)
    ix.reweight(ix.N)
    for got in (mid, after, ix.expand_wildcards(patterns)):
        assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes()
    assert ix.wildcard_stats() == stats


def test_device_entry(sme, small):
    ix, terms = small
    for patterns in (W.PATTERNS, ["absent"], []):
        off, ids = ix.expand_wildcards(patterns)
        d_off, d_ids, total = ix.expand_wildcards_device(patterns)
        assert total == off[-1] and d_off
        got_off = np.zeros(len(patterns) + 1, np.int64)
        sme.memcpy(got_off.ctypes.data, d_off, got_off.nbytes)
        got_ids = np.zeros(max(total, 1), np.int32)
        if total:
            sme.memcpy(got_ids.ctypes.data, d_ids, 4 * total)
        assert np.array_equal(got_off, off) and np.array_equal(got_ids[:total], ids)


def test_refusals(sme, built):
    corpus, ids = _fuzz()
    cg = sme.Context(2, 2).build_chargram(corpus)
    ctx2 = sme.Context(2, 2)
    ctx2.load_docno_mapping(sme.TrecDocnoMapping.write(ids))
    k2 = ctx2.build(corpus)
    import torch
    sizes = built.pack_pieces(1)
    blob = torch.empty(max(sum(sizes), 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    built.pack_pieces(1, blob.data_ptr())
    merged = built.ctx.merge_pieces(blob.data_ptr(), sizes)
    for obj, word in ((cg, "CharKGramTermIndexer"), (k2, "K = 2"), (merged, "records-only")):
        for call in (lambda: sme.Index.expand_wildcards(obj, ["a*"]), lambda: sme.Index.wildcard_stats(obj),
                     lambda: sme.Index.prepare_wildcards(obj), lambda: sme.Index.expand_wildcards_device(obj, ["a*"])):
            with pytest.raises(sme.SmeError) as e:
                call()
            assert e.value.code == SME_EINVAL and word in str(e.value), str(e.value)
    _check(built, ["appl*"])


def _end_to_end(sme, ix):
    terms = ix.terms()
    fw = sme.IntDocVectorsForwardIndex(ix)
    fw.get_wildcard(["appl*", "running"])
    plain = [int(t) for t in ix.lookup(ix.ctx.process_content("running")) if t >= 0]
    want = plain + W.matches("appl*", terms)
    assert plain and len(want) > len(plain) and fw._terms == want
    dn, sc = ix.query_topk(np.array(want, np.int32), np.array([0, len(want)], np.int64), 10)
    assert fw.rank(10) == [int(d) for d in dn[0] if d >= 0] and len(fw.rank(10)) > 0
    dn2, sc2 = ix.query_topk(np.array(fw._terms, np.int32), np.array([0, len(fw._terms)], np.int64), 10)
    assert dn2.tobytes() == dn.tobytes() and sc2.tobytes() == sc.tobytes()
    # upper-case wildcard words are lower-cased; a term reached twice counts twice
    fw.get_wildcard(["APPL*", "appl*"])
    assert fw._terms == 2 * W.matches("appl*", terms)
    fw.get_wildcard(["nosuchterm*", "zzzzzz"])
    assert fw._terms == [] and fw.rank(10) == []


def test_end_to_end(sme, built):
    _end_to_end(sme, built)
    parts = [bytes(built.partition_records(p)) for p in range(built.ctx.num_partitions)]
    _end_to_end(sme, sme.Context(1, 3).load_records(parts))
