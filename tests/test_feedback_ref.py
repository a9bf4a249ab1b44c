"""The two restatements of relevance feedback in feedback_ref.py agree: counting a
set's records' streams (a) gives, for every set the device is tested with, what
restricting the oracle's K = 1 posting lists to the set gives (b).  No device."""
import pytest

import feedback_ref as F


@pytest.mark.parametrize("name", F.NAMES)
def test_streams_equal_restricted_postings(name):
    fb = F.reference(name)
    terms = F.oracle_terms(name)
    sets = F.standard_sets(fb)
    nonempty = 0
    for s in sets:
        got, positions, missing = fb.count(s)
        assert got == F.oracle_count(terms, s), s[:8]
        assert positions == sum(f for f, _ in got.values())
        assert missing == sum(1 for d in fb.members(s) if d not in fb.by_docno)
        nonempty += bool(got)
    assert nonempty >= 16
    # the index's own document frequencies are the oracle's posting counts
    df = {g[0]: len(p) for g, _, _, p in terms if g != (" ",)}
    assert df == fb.df


def test_sets_reach_their_cases():
    for name in F.NAMES:
        fb = F.reference(name)
        sets = F.standard_sets(fb)
        assert [] in sets and [-1, -1, -1] in sets
        assert any(len(s) == 1 for s in sets) and any(len(s) == 2 for s in sets) and any(len(s) == 10 for s in sets)
        assert sorted(d for s in sets if len(s) > 10 for d in s) == sorted(fb.by_docno)  # every docno, runs of 1024
        assert any(len(s) > len(fb.members(s)) > 1 for s in sets)  # a repeated docno
        assert any(fb.count(s)[2] > 0 and fb.count(s)[0] for s in sets)  # absent docnos beside a present one
    # the fuzz corpus has docno 0 and negative docnos in several records each
    fb = F.reference("fuzz")
    shared = [d for d in fb.by_docno if d < 0 and len(fb.by_docno[d]) > 1]
    assert len(fb.by_docno[0]) > 1 and shared
    assert any(0 in s and any(d in shared for d in s) for s in F.standard_sets(fb))
    # the split corpus holds the record with 100 distinct body terms
    big = F.reference("split").st.records[F.BIG_RECORD]
    assert len(set(big[1])) >= 100
