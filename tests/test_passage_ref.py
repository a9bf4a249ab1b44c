"""The passages restatement the GPU tests trust (passage_ref.py: windows slid along a
record) held to an independent brute force that looks at every window on its own with a
set and a counter, on the c1, split and fuzz corpora of feedback_ref.corpus; and to a few
windows written out by hand."""
import random

import pytest

import feedback_ref as F
import passage_ref as PR

WIDTHS = (1, 2, 5, 64, 256)


def _ref(name):
    fb = F.reference(name)
    ids = {t: i for i, t in enumerate(sorted(fb.df))}  # (any numbering serves here)
    return PR.Ref(fb, ids), ids


def _queries(fb, ids, rng):
    by_df = sorted(fb.df, key=lambda t: (-fb.df[t], t))
    common, rare = by_df[:30], [t for t in by_df if fb.df[t] == 1][:200]
    qs = [[ids[common[0]]], [ids[t] for t in common[:3]], [ids[t] for t in rng.sample(common, 6)],
          [ids[t] for t in rng.sample(rare, min(4, len(rare)))] + [ids[common[1]]],
          [ids[common[2]], -1, ids[common[2]], ids[common[5]], -1], [], [-1]]
    qs.append([ids[t] for t in rng.sample(by_df[:400], min(64, len(by_df)))])
    return qs


@pytest.mark.parametrize("idf_mode", [0, 1])
@pytest.mark.parametrize("name", F.NAMES)
def test_sliding_equals_brute_force(name, idf_mode):
    ref, ids = _ref(name)
    rng = random.Random(3)
    docnos = sorted(ref.streams)
    several = [d for d in docnos if len(ref.streams[d]) > 1]
    cands = sorted(set(rng.sample(docnos, 25) + several[:6] + docnos[:2] + docnos[-2:])) + [max(docnos) + 9]
    if name == "fuzz":
        assert several and 0 in ref.streams and min(docnos) < 0
    seen = set()
    for listed in _queries(ref.fb, ids, rng):
        slots = tuple(PR.slots_of(listed))
        idfs = ref.idfs(slots, idf_mode)
        for width in WIDTHS:
            for d in cands:
                got = ref.best(slots, d, width, idf_mode)
                assert got == PR.brute(ref.streams, list(slots), d, width, idfs), (listed, d, width)
                seen.add((got.rec > 0, got.start > 0, got.hits > 1, bin(got.mask).count("1") > 1, got.len < width))
    assert len(seen) >= (8 if name == "fuzz" else 6)  # the cases are not all alike


def test_by_hand():
    class FB:  # three records: docno 4 twice, docno 9 once
        N = 3
        by_docno = {4: [["c", "x", "a", "x"], ["a", "b", "x"]], 9: [[]]}
        df = {"a": 1, "b": 1, "c": 1, "x": 1}

        def idf(self, term, idf_mode):
            return {"a": 0.5, "b": 0.25, "c": 0.0, "x": 9.0}[term]

    ids = {"a": 0, "b": 1, "c": 2, "x": 3}
    ref = PR.Ref(FB(), ids)
    q = ([1, -1, 0, 1, 2], [4, 9, 11])  # slots: b 0, a 1, c 2
    assert PR.slots_of(q[0]) == [1, 0, 2]
    res, st = ref.run([q], 2, with_terms=True)
    # docno 4: record 0's windows cover {c}, {a}, {a}; record 1's [0, 2) covers a and b: 0.25 + 0.5
    assert res.docno.tolist() == [4, 9, 11] and res.rec.tolist() == [1, 0, -1] and res.start.tolist() == [0, 0, 0]
    assert res.len.tolist() == [2, 0, 0] and res.hits.tolist() == [2, 0, 0] and res.mask.tolist() == [3, 0, 0]
    assert res.score.tolist() == [0.25 + 0.5, 0.0, 0.0]
    assert res.win_off.tolist() == [0, 2, 2, 2] and res.win_term.tolist() == [0, 1] and res.win_slot.tolist() == [1, 0]
    assert st == {"candidates": 3, "with_record": 2, "positions": 7, "kept": 3}
    # width 1: a alone (0.5) beats b (0.25); the first a is record 0's position 2
    res, _ = ref.run([q], 1)
    assert (res.rec[0], res.start[0], res.mask[0], res.score[0]) == (0, 2, 2, 0.5) and res.win_off.tolist() == [0]
    # cover decides where the idf is 0.0: only c listed, record 0 start 0 holds it
    res, _ = ref.run([([2], [4])], 3)
    assert (res.rec[0], res.start[0], res.hits[0], res.mask[0], res.score[0]) == (0, 0, 1, 1, 0.0)
    # min_cover, the orders and the cut
    two = [q, ([0], [4, 9])]
    res, st = ref.run(two, 2, min_cover=1, order=1, m=1)
    assert res.res_off.tolist() == [0, 1, 2] and res.docno.tolist() == [4, 4] and st["kept"] == 2
    res, _ = ref.run(two, 2, min_cover=0, order=1)
    assert res.docno.tolist() == [4, 9, 11, 4, 9]
    with pytest.raises(AssertionError):
        ref.run([([0], [9, 4])], 2)
