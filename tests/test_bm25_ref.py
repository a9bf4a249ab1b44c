"""The BM25 restatement (bm25_ref.py) against a brute-force scorer over a dict of
documents, on random small collections, and three results written out by hand."""
import math
import random

import numpy as np

import bm25_ref as R


def _collection(rng, n_docs, V, lo=-3):
    """{docno: {term: tf}} with some docnos missing, some negative, and the CSR of it."""
    docs = {}
    for d in range(lo, lo + n_docs):
        if rng.random() < 0.15:
            continue
        terms = rng.sample(range(V), rng.randint(1, min(V, 6)))
        docs[d] = {t: rng.choice([1, 1, 2, 3, 9, 40]) for t in terms}
    off, dn, tf = [0], [], []
    for t in range(V):
        for d in sorted(docs):
            if t in docs[d]:
                dn.append(d)
                tf.append(docs[d][t])
        off.append(len(dn))
    return docs, R.Ref(off, dn, tf)


def _brute(docs, V, terms, k, k1, b):
    D = len(docs)
    dl = {d: sum(v.values()) for d, v in docs.items()}
    avgdl = float(sum(dl.values())) / float(D)
    df = [sum(1 for v in docs.values() if t in v) for t in range(V)]
    rows = []
    for d, v in docs.items():
        s, hit = 0.0, False
        for t in terms:
            if t >= 0 and t in v:
                norm = k1 * ((1.0 - b) + b * (float(dl[d]) / avgdl))
                s += math.log(1.0 + ((float(D - df[t]) + 0.5) / (float(df[t]) + 0.5))) * \
                    ((float(v[t]) * (k1 + 1.0)) / (float(v[t]) + norm))
                hit = True
        if hit:
            rows.append((-s, d))
    rows.sort()
    rows = rows[:k]
    return [d for _, d in rows] + [-1] * (k - len(rows)), [-s for s, _ in rows] + [0.0] * (k - len(rows))


def test_against_brute_force():
    rng = random.Random(5)
    for trial in range(30):
        V = rng.randint(3, 12)
        docs, ref = _collection(rng, rng.randint(4, 60), V)
        if not docs:
            continue
        assert ref.D == len(docs) and ref.L == sum(sum(v.values()) for v in docs.values())
        for d, v in docs.items():
            assert ref.doc_length(d) == sum(v.values())
        for _ in range(12):
            terms = [rng.choice(list(range(V)) + [-1]) for _ in range(rng.randint(0, 6))]
            k1, b = rng.choice([(1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (0.9, 1.0)])
            k = rng.choice([1, 3, 10, 100])
            od, os = ref.topk(terms, k, k1, b)
            wd, ws = _brute(docs, V, terms, k, k1, b)
            assert od.tolist() == wd, (trial, terms)
            assert [R.bits(x) for x in os] == [R.bits(x) for x in ws], (trial, terms)


def _tiny():
    # term 0 = a, 1 = b;  d1: a,  d2: a a b,  d3: b b b   ->  dl 1, 3, 3;  D 3, L 7
    return R.Ref([0, 2, 4], [1, 2, 2, 3], [1, 2, 1, 3])


def test_by_hand_no_saturation():
    """k1 = 0: every posting weighs its idf, ties go to the smaller docno."""
    ref = _tiny()
    assert (ref.D, ref.L, ref.dl.tolist()) == (3, 7, [1, 3, 3])
    idf = math.log(1.0 + (1.0 + 0.5) / (2.0 + 0.5))  # df 2 of D 3, both terms
    od, os = ref.topk([0], 3, 0.0, 0.75)
    assert od.tolist() == [1, 2, -1] and os.tolist() == [idf, idf, 0.0]


def test_by_hand_two_terms():
    ref = _tiny()
    idf = math.log(1.0 + (1.0 + 0.5) / (2.0 + 0.5))
    avgdl = 7.0 / 3.0
    n1 = 1.2 * ((1.0 - 0.75) + 0.75 * (1.0 / avgdl))
    n3 = 1.2 * ((1.0 - 0.75) + 0.75 * (3.0 / avgdl))
    s1 = 0.0 + idf * ((1.0 * (1.2 + 1.0)) / (1.0 + n1))
    s2 = (0.0 + idf * ((2.0 * (1.2 + 1.0)) / (2.0 + n3))) + idf * ((1.0 * (1.2 + 1.0)) / (1.0 + n3))
    s3 = 0.0 + idf * ((3.0 * (1.2 + 1.0)) / (3.0 + n3))
    assert s2 > s3 > s1 and s3 < 3.0 * s1  # tf saturates: three b weigh less than three times one a
    od, os = ref.topk([0, 1], 4, 1.2, 0.75)
    assert od.tolist() == [2, 3, 1, -1]
    assert [R.bits(x) for x in os] == [R.bits(x) for x in (s2, s3, s1, 0.0)]


def test_by_hand_duplicates_and_cut():
    """A term listed twice counts twice, -1 is skipped, b = 0 drops the length, k cuts."""
    ref = _tiny()
    idf = math.log(1.0 + (1.0 + 0.5) / (2.0 + 0.5))
    w3 = idf * ((3.0 * (2.0 + 1.0)) / (3.0 + 2.0 * ((1.0 - 0.0) + 0.0 * (3.0 / (7.0 / 3.0)))))
    od, os = ref.topk([1, -1, 1], 1, 2.0, 0.0)
    assert od.tolist() == [3] and R.bits(os[0]) == R.bits((0.0 + w3) + w3)
    od, os = ref.topk([-1], 2, 1.2, 0.75)
    assert od.tolist() == [-1, -1] and os.tolist() == [0.0, 0.0]
    od, _ = R.Ref([0, 0], [], []).topk([0], 2)  # no document at all
    assert od.tolist() == [-1, -1]


def test_batch_and_run():
    ref = _tiny()
    ids, off = R.batch([[0], [], [1, 0]])
    assert ids.tolist() == [0, 1, 0] and off.tolist() == [0, 1, 1, 3]
    od, os = ref.run(ids, off, 2)
    assert od.shape == (3, 2) and od[1].tolist() == [-1, -1]
    assert np.array_equal(od[2], ref.topk([1, 0], 2)[0])
