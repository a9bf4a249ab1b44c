"""The structured-query restatement (structq_ref.py) against answers derived by hand
on a six-record corpus, so the yardstick of test_gpu_structq.py is pinned without
the library.  Tokens are the term ids themselves.

    docno 1: a b c      docno 4: b a
    docno 2: a c b      docno 5: c d
    docno 3: a b a b    docno 6: a b d

    "a b" (#od:1)   docs 1 (freq 1), 3 (freq 2), 6 (freq 1)       df 3
    #uw:3(a c)      docs 1 (freq 1), 2 (freq 1)                   df 2
    #od:2(a c)      docs 1, 2 (freq 1)                            df 2
    a: docs 1 2 3(tf 2) 4 6  df 5    b: the same    c: docs 1 2 5  df 3    d: docs 5 6  df 2
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import structq_ref as SR

A, Bt, Cc, D = range(4)
RECORDS = [(1, [A, Bt, Cc]), (2, [A, Cc, Bt]), (3, [A, Bt, A, Bt]), (4, [Bt, A]), (5, [Cc, D]), (6, [A, Bt, D])]
N = 6
REQ, EXC = False, True
AB = ([A, Bt], 1, 1)
UW = ([A, Cc], 2, 3)


def T(t):
    return ([t], 0, 0)


def idf(mode, df):
    return math.log10(float(N // (1 if mode == 0 else df)))


def lut(f):
    return 1.0 + math.log(float(f))


def _csr(mode):
    """The query-side CSR of RECORDS as the weight pass forms it."""
    off, dn, w = [0], [], []
    for t in range(4):
        tf = {}
        for d, s in RECORDS:
            if s.count(t):
                tf[d] = s.count(t)
        for d in sorted(tf):
            dn.append(d)
            w.append(lut(tf[d]) * idf(mode, len(tf)))
        off.append(len(dn))
    return np.array(off, np.int64), np.array(dn, np.int32), np.array(w, np.float64)


def _run(mode, queries, order=0, m=0, **kw):
    st = SimpleNamespace(records=RECORDS, N=N)
    return SR.run(st, _csr(mode), queries, order, m, mode, **kw)


def _one(mode, groups):
    (off, dn, sc), _, _, _ = _run(mode, [groups])
    return dict(zip(dn.tolist(), sc.tolist()))


@pytest.mark.parametrize("mode", [0, 1])
def test_leaf_lists(mode):
    _, _, _, lists = _run(mode, [[([AB], REQ)], [([UW, ([A, Cc], 1, 2)], REQ)], [([([A, -1], 1, 1), ([], 2, 4)], REQ)]])
    off, dn, fq, sc = lists
    assert off.tolist() == [0, 3, 5, 7, 7, 7] and dn.tolist() == [1, 3, 6, 1, 2, 1, 2] and fq.tolist() == [1, 2, 1, 1, 1, 1, 1]
    assert sc.tolist() == [lut(1) * idf(mode, 3), lut(2) * idf(mode, 3), lut(1) * idf(mode, 3)] + [lut(1) * idf(mode, 2)] * 4


@pytest.mark.parametrize("mode", [0, 1])
def test_excluded_phrase(mode):
    wa = lut(1) * idf(mode, 5)
    assert _one(mode, [([T(A)], REQ), ([AB], EXC)]) == {2: 0.0 + wa, 4: 0.0 + wa}
    # the excluded leaf adds nothing where it is absent, and pure negation matches nothing
    assert _one(mode, [([AB], EXC)]) == {}
    assert _one(mode, []) == {}


@pytest.mark.parametrize("mode", [0, 1])
def test_or_group_of_a_term_and_a_window(mode):
    wd, vu = lut(1) * idf(mode, 2), lut(1) * idf(mode, 2)
    assert _one(mode, [([T(D), UW], REQ)]) == {1: vu, 2: vu, 5: wd, 6: wd}
    assert _one(mode, [([UW, T(D)], REQ)]) == {1: vu, 2: vu, 5: wd, 6: wd}
    # AND-ed with c: listed order (d | uw) then c
    wc = lut(1) * idf(mode, 3)
    assert _one(mode, [([T(D), UW], REQ), ([T(Cc)], REQ)]) == {1: vu + wc, 2: vu + wc, 5: wd + wc}


@pytest.mark.parametrize("mode", [0, 1])
def test_duplicate_leaf_and_listed_order(mode):
    v1, v2 = lut(1) * idf(mode, 3), lut(2) * idf(mode, 3)
    assert _one(mode, [([AB, AB], REQ)]) == {1: v1 + v1, 3: v2 + v2, 6: v1 + v1}
    wd, wb = lut(1) * idf(mode, 2), lut(1) * idf(mode, 5)
    assert _one(mode, [([AB], REQ), ([T(D)], REQ)]) == {6: v1 + wd}
    assert _one(mode, [([T(Bt)], REQ), ([AB], REQ), ([T(D)], REQ)]) == {6: (wb + v1) + wd}
    # a one-term ordered leaf (any width) is the term leaf
    for width in (1, 7):
        assert _one(mode, [([([Cc], 1, width)], REQ)]) == _one(mode, [([T(Cc)], REQ)])


def test_order_cut_and_counts():
    qs = [[([AB], REQ)], [], [([T(A)], REQ), ([UW], REQ)], [([T(D)], REQ), ([AB], EXC)]]
    (off, dn, sc), cands, total, _ = _run(0, qs, 0, 0)
    assert off.tolist() == [0, 3, 3, 5, 6] and dn.tolist() == [1, 3, 6, 1, 2, 5]
    assert (cands, total) == (3 + 2 + 2, 6)  # the drivers: the phrase, the window (2 < 5), d
    (off, dn, sc), cands, total, _ = _run(0, qs, 1, 1, first_driver=True)
    assert off.tolist() == [0, 1, 1, 2, 3] and dn.tolist() == [3, 1, 5]
    assert sc[0] == lut(2) * idf(0, 3) and (cands, total) == (3 + 5 + 2, 6)
    assert off.dtype == np.int64 and dn.dtype == np.int32 and sc.dtype == np.float64


def test_another_n_and_term_strings():
    """N of the leaves' idf is the caller's; term_of maps ids to the streams' tokens."""
    st = SimpleNamespace(records=[(d, ["t%d" % t for t in s]) for d, s in RECORDS], N=N)
    (off, dn, sc), _, _, _ = SR.run(st, _csr(1), [[([AB], REQ)]], 0, 0, 1, N=60, term_of=lambda t: "t%d" % t)
    assert dn.tolist() == [1, 3, 6] and sc[1] == lut(2) * math.log10(float(60 // 3))
