"""near_ref.py, the brute-force restatement the proximity-query tests expect from,
held to the oracle chain: its ordered window of width 1 is phrase_ref's phrase
match (itself the oracle's K = m index, test_phrase_ref.py) for every gram of 1..3
terms of the fuzz corpus and of the c1 sample; both kinds are monotone in the
width; and an unordered window at or past the record's length is "one record holds
all the terms".  No device."""
import functools
import os

import pytest

import common
import near_ref as NR
import oracle_lib as O
import phrase_ref as P

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _streams(name):
    if name == "c1":
        corpus = open(os.path.join(G, "c1_sample_trec.xml"), "rb").read()
        mapping = open(os.path.join(G, "c1_sample_mapping.bin"), "rb").read()
    else:
        corpus, ids = common.fuzz_corpus(7, 300)
        mapping = O.write_mapping(ids)
    return P.Streams(corpus, mapping)


@pytest.mark.parametrize("name", ["fuzz", "c1"])
def test_ordered_width_1_is_the_phrase(name):
    st = _streams(name)
    # one pass per record over its own grams (every gram of the corpus is one of some
    # record): the gram's count by both restatements
    seen = 0
    for m in (1, 2, 3):
        grams = st.grams(m)
        by_rec = {}
        for d, s in st.records:
            at = NR.where(s)
            for g in {tuple(s[i:i + m]) for i in range(len(s) - m + 1)}:
                by_rec.setdefault(g, {}).setdefault(d, 0)
                by_rec[g][d] += NR.count_ordered(s, list(g), 1, at)
        assert by_rec == grams, m
        seen += len(grams)
        for g in list(grams)[:25]:  # and through match(), record filter included
            assert NR.match(st, list(g), 1, True) == st.match(list(g)) == grams[g], g
    assert seen > 1000


def _sample_queries(st, n):
    """Term tuples drawn from the records themselves: pairs and triples of terms of
    one record, in and out of stream order, some with a repeat."""
    out = []
    for d, s in st.records:
        if len(s) >= 6 and len(out) < n:
            out += [(s[0], s[3]), (s[4], s[1]), (s[1], s[2], s[5]), (s[5], s[0], s[0]), (s[2],)]
    return out[:n]


def test_monotone_in_the_width():
    st = _streams("fuzz")
    widths = (1, 2, 3, 5, 8, 64, 2 ** 31 - 1)
    grew = 0
    for q in _sample_queries(st, 60):
        for ordered in (True, False):
            prev = {}
            for N in widths:
                cur = NR.match(st, list(q), N, ordered)
                assert set(prev) <= set(cur) and all(cur[d] >= f for d, f in prev.items()), (q, N, ordered)
                grew += cur != prev
                prev = cur
    assert grew > 100


def test_unordered_past_the_record_length_is_containment():
    st = _streams("fuzz")
    longest = max(len(s) for _, s in st.records)
    for q in _sample_queries(st, 60):
        T = set(q)
        want = {}
        for d, s in st.records:
            if T <= set(s):
                # every position on a query term from the one that completes the set on
                first = max(s.index(t) for t in T)
                want[d] = want.get(d, 0) + sum(1 for e in range(first, len(s)) if s[e] in T)
        for N in (longest, longest + 1, 2 ** 31 - 1):
            assert NR.match(st, list(q), N, False) == want, (q, N)
        assert set(want) == {d for d, s in st.records if T <= set(s)} and want


def test_named_cases():
    od, uw = NR.count_ordered, NR.count_unordered
    a, b, c, x = "a", "b", "c", "x"
    assert od([a, b, b, x, c], [a, b, c], 2) == 1 and od([a, b, c, b], [a, b, c], 3) == 1  # not greedy
    assert od([a, x, x, b], [a, b], 3) == 1 and od([a, x, x, b], [a, b], 2) == 0
    assert od([a, x, a, a], [a, a], 2) == 2 and od([b, a], [a, b], 9) == 0
    assert od([a, b, b], [a, b], 2) == 2 and od([a, a, b], [a, b], 2) == 1  # distinct ends
    assert od([], [a], 1) == 0 and od([a], [], 1) == 0 and od([a, x, a], [a], 1) == 2
    assert uw([a, x, b], [b, a], 3) == 1 and uw([a, x, b], [a, b], 2) == 0
    assert uw([a, b, a], [a, b], 2) == 2 and uw([a, x, b], [a, b, a], 3) == 1  # the set
    assert uw([a, b, c], [a, b, c], 2) == 0 and uw([a, b], [a, b], 2 ** 31 - 1) == 1  # N < |T|; clipped
    assert uw([], [a], 1) == 0 and uw([a], [], 1) == 0


def test_run_shapes():
    st = _streams("fuzz")
    q = _sample_queries(st, 5)
    qs = [(list(q[0]), 5, True), ([], 3, False), ([q[1][0], None], 3, False), (list(q[2]), 2 ** 31 - 1, False)]
    off, dn, fq, sc = NR.run(st, qs, 1, 0, 1)
    assert off[0] == 0 and off[1] > 0 and off[2] == off[1] == off[3] and off[4] > off[3]
    assert len(dn) == len(fq) == len(sc) == off[-1] and (fq > 0).all()
    cut = NR.run(st, qs, 1, 1, 1)
    assert cut[0].tolist() == [0, 1, 1, 1, 2] and cut[3][0] == sc[0]
