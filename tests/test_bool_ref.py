"""The Boolean restatement (bool_ref.py) against answers derived by hand on a
six-document example, so the yardstick of test_gpu_bool.py is pinned without the
library.

    term 0 "a": docs 1 2 3 4    weights 1 2 3 4
    term 1 "b": docs 2 4 6      weights 0.5 0.25 0.125
    term 2 "c": docs 3 4 5      weights 10 20 30
    term 3 "d": no postings
    term 4 "e": doc 4           weight 100
    term 5 "f": docs 5 6        weights 7 7
"""
import numpy as np

import bool_ref as B

OFF = [0, 4, 7, 10, 10, 11, 13]
DOCNO = [1, 2, 3, 4, 2, 4, 6, 3, 4, 5, 4, 5, 6]
W = [1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 0.125, 10.0, 20.0, 30.0, 100.0, 7.0, 7.0]
A, Bt, Cc, D, E, F = range(6)
REQ, EXC = False, True


def _ref():
    return B.Ref(np.array(OFF, np.int64), np.array(DOCNO, np.int32), np.array(W, np.float64))


def test_and_or_not():
    r = _ref()
    assert r.matches([([A], REQ), ([Bt], REQ)]) == {2: 2.5, 4: 4.25}
    # (b OR c) AND a: slots in listed order b, c, a
    assert r.matches([([Bt, Cc], REQ), ([A], REQ)]) == {2: 0.5 + 2.0, 3: 10.0 + 3.0, 4: (0.25 + 20.0) + 4.0}
    assert r.matches([([A], REQ), ([Cc], EXC)]) == {1: 1.0, 2: 2.0}
    assert r.matches([([A], REQ), ([Cc, Bt], EXC)]) == {1: 1.0}
    assert r.matches([([A], REQ), ([Bt], REQ), ([Cc], REQ), ([E], REQ)]) == {4: ((4.0 + 0.25) + 20.0) + 100.0}
    assert r.matches([([A, Bt, Cc, F], REQ)]).keys() == {1, 2, 3, 4, 5, 6}


def test_queries_that_match_nothing():
    r = _ref()
    assert r.matches([]) == {}
    assert r.matches([([Cc], EXC)]) == {}  # exclusions only: pure negation is not offered
    assert r.matches([([A], REQ), ([D], REQ)]) == {}  # a required group without a posting
    assert r.matches([([A], REQ), ([-1], REQ)]) == {}
    assert r.matches([([A], REQ), ([], REQ)]) == {}
    assert r.matches([([A], REQ), ([A], EXC)]) == {}  # required and excluded
    assert r.matches([([A, -1, D], REQ), ([-1, D], EXC)]) == {1: 1.0, 2: 2.0, 3: 3.0, 4: 4.0}
    assert r.matches([([Bt], REQ), ([F], REQ), ([E], REQ)]) == {}
    for q in ([], [([Cc], EXC)], [([A], REQ), ([D], REQ)]):
        assert r.driver(q) is None and r.driver(q, first=True) is None


def test_repeated_terms_count_twice():
    r = _ref()
    assert r.matches([([Bt, Bt], REQ), ([Bt], REQ)]) == {2: 1.5, 4: 0.75, 6: 0.375}
    assert r.matches([([A, Bt], REQ), ([Bt, A], REQ)])[4] == ((4.0 + 0.25) + 0.25) + 4.0


def test_driver_rule():
    r = _ref()
    assert r.driver([([A], REQ), ([Bt], REQ)]) == (1, 3)
    assert r.driver([([A], REQ), ([Bt], REQ)], first=True) == (0, 4)
    assert r.driver([([Bt, Cc], REQ), ([A], REQ)]) == (1, 4)
    assert r.driver([([Bt], REQ), ([Cc], REQ)]) == (0, 3)  # a tie goes to the lower index
    assert r.driver([([E], EXC), ([A], REQ), ([Bt, Bt], REQ)]) == (1, 4)  # an excluded group never drives
    assert r.driver([([Bt, Bt], REQ)]) == (0, 6)


def test_order_cut_and_counts():
    r = _ref()
    qs = [[([Bt, Cc], REQ), ([A], REQ)], [], [([F], REQ)], [([A], REQ), ([Bt], REQ)]]
    (off, dn, sc), cands, total = r.run(qs, order=0, m=0)
    assert off.tolist() == [0, 3, 3, 5, 7] and dn.tolist() == [2, 3, 4, 5, 6, 2, 4]
    assert sc.tolist() == [2.5, 13.0, 24.25, 7.0, 7.0, 2.5, 4.25]
    assert (cands, total) == (4 + 2 + 3, 7)
    (off, dn, sc), cands, total = r.run(qs, order=1, m=2, first_driver=True)
    # score descending, equal scores by docno; the counts are taken before the cut
    assert off.tolist() == [0, 2, 2, 4, 6] and dn.tolist() == [4, 3, 5, 6, 4, 2]
    assert sc.tolist() == [24.25, 13.0, 7.0, 7.0, 4.25, 2.5]
    assert (cands, total) == (6 + 2 + 4, 7)
    assert off.dtype == np.int64 and dn.dtype == np.int32 and sc.dtype == np.float64
    (off, dn, _), _, _ = r.run(qs, order=1, m=1)
    assert off.tolist() == [0, 1, 1, 2, 3] and dn.tolist() == [4, 5, 4]
