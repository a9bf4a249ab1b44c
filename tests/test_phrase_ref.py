"""phrase_ref.py, the Python restatement the phrase-query tests expect from, held to
the reference semantics: the windows of m terms over its per-record streams are
exactly the grams of the oracle's K = m index, posting for posting, for m = 1, 2, 3
on a fuzz corpus with the quirks on (docno 0, duplicate docids, negative docnos)."""
import functools

import pytest

import common
import oracle_lib as O
import phrase_ref as P


@functools.lru_cache(maxsize=None)
def _fuzz():
    corpus, ids = common.fuzz_corpus(7, 300)
    mapping = O.write_mapping(ids)
    return corpus, mapping, P.Streams(corpus, mapping)


def test_quirks_are_present():
    _, _, st = _fuzz()
    docnos = [d for d, _ in st.records]
    assert docnos.count(0) > 1  # records without DOCNO
    assert min(docnos) < 0  # a docid missing from the mapping
    assert any(docnos.count(d) > 1 for d in set(docnos) if d > 0)  # a duplicate docid
    # a DOCNO's tokens are part of the stream: FZ000007-31 gives fz000007, 31
    assert sum(1 for _, s in st.records if len(s) >= 2 and s[0].startswith("fz0") and s[1].isdigit()) > 200


@pytest.mark.parametrize("m", [1, 2, 3])
def test_windows_are_the_oracles_grams(m):
    corpus, mapping, st = _fuzz()
    ref = O.OracleIndex(corpus, mapping, m, 1)
    want = {t[0]: dict(t[3]) for t in ref.terms() if t[0] != (" ",)}
    got = st.grams(m)
    assert set(got) == set(want)  # no gram missing, none extra
    for g, posts in want.items():
        assert got[g] == posts, g
    # and the per-phrase count agrees with the windows
    for g in list(want)[:200]:
        assert st.match(list(g)) == want[g], g


def test_phrase_count_cases():
    c = P.phrase_count
    assert c([], ["a"]) == 0 and c(["a"], []) == 0
    assert c(["a", "a", "a"], ["a", "a"]) == 2  # overlaps all count
    assert c(["a", "b", "a", "b", "a"], ["a", "b", "a"]) == 2
    assert c(["a", "b"], ["a", "b", "c"]) == 0 and c(["a", "b", "c"], ["a", "b", "c"]) == 1
    assert c(["x", "a", "b"], ["a", "b"]) == 1 and c(["a", "b", "x"], ["a", "b"]) == 1


def test_docno_lookup():
    ids = ["A1", "B2", "C3"]
    assert P.get_docno(ids, "") == 0 and P.get_docno(ids, "A1") == 1 and P.get_docno(ids, "C3") == 3
    assert P.get_docno(ids, "B0") == -3 and P.get_docno(ids, "ZZ") == -5
    assert P.get_docid(b"<DOC>\n<DOCNO> FZ1-02 </DOCNO>\n</DOC>") == "FZ1-02"
    assert P.get_docid(b"<DOC> none </DOC>") == ""
