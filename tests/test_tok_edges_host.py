"""The edge-corpus generator (tests/tok_edges.py) checked on the CPU, before any
device run: its placements and declared paths, its vocabularies, the expected
tokens of every construct on two independent restatements of the tokenizer, and
the marker expectations against the oracle's own build."""
import functools

import pytest

import oracle_lib as O
import pyref_tokenize as P
import tok_edges as T


@pytest.mark.parametrize("mis", T.MIS)
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_placement(family, mis):
    """Every construct's byte j on its edge, the declared fast / slow split equal to
    the restated lt_simple, at most 2 MB, docids unique and all in the mapping."""
    c = T.corpus(family, mis)
    assert c.check()
    assert len(c.buf) <= 2 * 1000 * 1000
    ids = c.docids()
    assert ids == sorted(set(ids)) and len(ids) == len(c.recs)
    m = c.mapping()
    assert int.from_bytes(m[:4], "big") == len(ids) and all(d.encode() in m for d in ids[:: max(1, len(ids) // 50)])
    placed = [r for r in c.recs if r.get("kind") in tuple("CWLS")]
    assert len(placed) >= 100 or family in ("comments_long", "window"), len(placed)
    waves = {(x + mis) % T.CHUNK // T.WAVE for x, kind, _ in c.anchors if kind == "W"}
    lanes = {(x + mis) % T.CHUNK // T.LANE for x, kind, _ in c.anchors if kind == "L"}
    if any(r.get("kind") == "W" for r in c.recs) and family != "comments_long":
        assert waves == {1, 2, 3}, waves  # every wave total of the block scans
    assert all(l % 64 for l in lanes)
    if len(placed) >= 100 and family != "comments_long":  # lane edges in every wave of the chunk
        assert len(lanes) >= 16 and {l // 64 for l in lanes} == {0, 1, 2, 3}, sorted(lanes)
    if family == "window":
        assert c.n_slow() == 400 and c.n_fast() == 2004


def test_edge_arithmetic():
    """next_edge / is_edge against the kernel's formula: chunk k of the workgroup
    begins at ((rs0 + mis) & ~15) - mis + k * CHUNK with rs0 = 0."""
    for mis in range(16):
        org = ((0 + mis) & ~15) - mis
        assert org == -mis
        for k in (1, 2, 7):
            c = org + k * T.CHUNK
            assert T.is_edge("C", c, mis) and T.next_edge("C", c - 5, mis) == c and T.next_edge("C", c, mis) == c
            assert not T.is_edge("W", c, mis) and not T.is_edge("L", c, mis)
            assert T.is_edge("W", c + T.WAVE, mis) and T.is_edge("L", c + 63 * T.LANE, mis)
            assert T.is_edge("S", c - T.CHUNK + T.STAGE, mis) and T.next_edge("S", c + 1, mis) == c + T.STAGE - T.CHUNK
            assert T.next_edge("L", c, mis) == c + T.LANE and T.next_edge("W", c + 1, mis) == c + T.WAVE
    assert T.cuts(5) == [0, 1, 2, 3, 4, 5] and T.cuts(20, (9,)) == [0, 1, 2, 3, 9, 17, 18, 19, 20]


def test_neighbour_corpora():
    for c, fast, slow in ((T.dense_lt(), 6, 2), (T.docid_window(), 1 + 16 * 63 + 16 * 20, 0)):
        assert c.check() and (c.n_fast(), c.n_slow()) == (fast, slow)
    c = T.docid_window()
    t = c.bytes()
    ends = set()
    for r in c.recs[1:]:  # </DOCNO> ends on every side of window byte 96, at every start offset, for mis 0 and 9
        assert r["re"] - r["rs"] >= T.MIN_FAST
        for mis in (0, 9):
            js = (r["rs"] + mis) & 15
            ends.add((js, js + t.index(b"</DOCNO>", r["rs"]) - r["rs"] + 8 <= T.DOC_WIN))
    assert ends == {(js, b) for js in range(16) for b in (False, True)}


def test_vocabularies_stem_to_themselves():
    """Filler, hidden and marker words: no stopwords, unchanged by the stemmer, so a
    marker's term is the marker."""
    words = T.FILL + T.HIDDEN + [b"zq", b"jq001", b"jq002"]
    words += [T.bef(n) for n in range(1, 2000, 7)] + [T.aft(n) for n in range(1, 2000, 7)]
    words += [b"v%06d" % k for k in range(0, 2400, 37)] + [b"x%07d" % k for k in range(0, 2400, 37)]
    assert len(set(T.FILL)) == 300 and min(len(w) for w in T.FILL) >= 5
    assert not set(T.FILL) & set(T.HIDDEN)
    got = O.process_content(b" ".join(words))
    assert got == [w.decode() for w in words]


def test_constructs_oracle_vs_pyref():
    """Every construct between markers, abutting and a space away, ~200 bytes of
    filler either side: the C oracle and the Python restatement agree on the
    tokens (the 40000-byte comment is left to its 20000-byte sibling: the
    restatement runs ~80 KB/s)."""
    total = 0
    for family in T.FAMILIES:
        c = T.corpus(family, 0)
        for ci, cons in sorted(c.constructs.items()):
            if len(cons) > 20000:
                continue
            text = c.fill(200) + b"befa" + cons + b"afta befs " + cons + b" afts" + c.fill(200)
            total += len(text)
            assert O.process_content(text) == P.process_content(text), (family, ci)
    assert total < 100 * 1000 * 2


@functools.lru_cache(maxsize=None)
def _oracle_terms(family):
    c = T.corpus(family, 0)
    ref = O.OracleIndex(c.bytes(), c.mapping(), 1, 1)
    return {t[0][0]: t[3] for t in ref.terms()}


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_oracle_markers(family):
    """The expectation the device is held to is sane by construction: in the
    oracle's build every case's markers have one posting (tf 1) in the case's
    document, and no hidden word is a term."""
    c = T.corpus(family, 0)
    terms = _oracle_terms(family)
    docno = {d: i + 1 for i, d in enumerate(c.docids())}
    n = 0
    for r in c.recs:
        for w in r["expect"]:
            assert terms.get(w.decode()) == [(docno[r["docid"]], 1)], (r["docid"], w)
            n += 1
        for w in r["hidden"]:
            assert w.decode() not in terms, (r["docid"], w)
    assert n >= 80


def test_oracle_markers_neighbours():
    for c in (T.dense_lt(), T.docid_window()):
        ref = O.OracleIndex(c.bytes(), c.mapping(), 1, 1)
        terms = {t[0][0]: t[3] for t in ref.terms()}
        docno = {d: i + 1 for i, d in enumerate(c.docids())}
        for r in c.recs:
            for w in r["expect"]:
                assert terms.get(w.decode()) == [(docno[r["docid"]], 1)], (r["docid"], w)
