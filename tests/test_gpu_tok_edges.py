"""The byte-parallel tokenizer (k_tok_fast) at its chunk, wave, lane and stage
edges, through the public build path, against the CPU oracle.

tests/tok_edges.py builds one corpus per construct family and misalignment, one
case per record, each case's construct cut by an edge at a known byte.  Here every
family is built

  * placed: tok_grid = 1 (one workgroup walks every fast record, so the chunk
    origin is the one the generator assumed) from device memory at a pointer
    that is `mis` past a 16-byte boundary, mis in {0, 1, 8, 15}, R = 3;
  * placed with K = 2, the only view of the ORDER of a record's tokens across
    an edge (K = 1 compares (term, tf) multisets per record);
  * unplaced: plain Context.build with the default grid, where every workgroup
    has its own origin and the edges fall wherever they fall.

Each build is held to oracle_lib.OracleIndex bit for bit (common.check_index), to
the generator's declared fast / slow record counts (profile counters
records_fast / records_slow: a case meant for k_tok_fast that took k_tok_slow
would test nothing) and to tok_attempts == 1; and, independent of the oracle, every
case's marker words have exactly one posting, in that case's document, with tf 1,
while no word hidden inside a span is in the vocabulary.  On a mismatch the docids
of the documents that differ are printed: they spell the cases.

Two neighbours: k_scan_lt's overflow path (more than 2048 '<' in one 16 KiB step)
and k_docno's 96-byte window at every record start offset.
"""
import functools

import pytest

import common
import oracle_lib as O
import tok_edges as T

pytestmark = pytest.mark.gpu
R = 3


@functools.lru_cache(maxsize=None)
def _ref(family, mis, K, R):
    c = T.corpus(family, mis)
    return O.OracleIndex(c.bytes(), c.mapping(), K, R)


def _doc_terms(parts):
    """{docno: sorted [(gram, tf)]} of a list of partition record streams."""
    d = {}
    for buf in parts:
        for gram, _, posts, _ in common.parse_records(bytes(buf)):
            if gram == (b" ",):
                continue
            for dn, tf in posts:
                d.setdefault(dn, []).append((gram, tf))
    return {k: sorted(v) for k, v in d.items()}


def differing_docids(ix, ref, R, ids):
    """Docids (sorted mapping `ids`) whose (gram, tf) multisets differ between the
    device's records and the oracle's."""
    got = _doc_terms([ix.partition_records(p) for p in range(R)])
    want = _doc_terms([ref.partition_bytes(p) for p in range(R)])
    bad = sorted(d for d in set(got) | set(want) if got.get(d) != want.get(d))
    return [ids[d - 1] if 1 <= d <= len(ids) else "docno %d" % d for d in bad]


def _check(ix, ref, c, K=1):
    try:
        common.check_index(ix, ref, R, K)
    except AssertionError as e:
        bad = differing_docids(ix, ref, R, c.docids())
        print("documents that differ from the oracle (%d): %s" % (len(bad), " ".join(bad)))
        raise AssertionError("%d documents differ from the oracle: %s ... (%s)" % (len(bad), " ".join(bad[:12]), e))


def _counters(ctx, c):
    prof = ctx.last_build_profile()
    assert (prof["records_fast"], prof["records_slow"]) == (c.n_fast(), c.n_slow()), prof
    assert prof["tok_attempts"] == 1, prof
    return prof


def _markers(ix, c):
    """Every expected word: one posting, in its case's document, tf 1; no hidden word."""
    off, dn, tf, _ = ix.csr()
    ids = c.docids()
    docno = {d: i + 1 for i, d in enumerate(ids)}
    words, where, hidden = [], [], set()
    for r in c.recs:
        for w in r["expect"]:
            words.append(w.decode())
            where.append(r["docid"])
        hidden.update(w.decode() for w in r["hidden"])
    t = ix.lookup(words)
    bad = []
    for w, d, i in zip(words, where, t.tolist()):
        if i < 0 or off[i + 1] - off[i] != 1 or dn[off[i]] != docno[d] or tf[off[i]] != 1:
            bad.append((d, w))
    assert not bad, "markers without exactly one posting (tf 1) in their document: %s" % bad[:20]
    hidden = sorted(hidden)
    if hidden:
        found = [w for w, i in zip(hidden, ix.lookup(hidden).tolist()) if i >= 0]
        assert not found, "words hidden inside spans reached the vocabulary: %s" % found[:20]


def _build_placed(sme, c, mis, K, tok_grid=1):
    """The corpus at `mis` bytes past a 16-byte boundary of device memory."""
    import torch
    data = c.bytes()
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    o = (-buf.data_ptr()) % 16 + mis
    buf[o:o + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert (buf.data_ptr() + o) % 16 == mis
    ctx = sme.Context(K, R)
    if tok_grid:
        ctx.set_option("tok_grid", tok_grid)
    ctx.load_docno_mapping(c.mapping())
    ix = ctx.build_device(buf.data_ptr() + o, len(data))
    ix._corpus = buf  # the text stays alive with the index
    return ctx, ix


@pytest.mark.parametrize("mis", T.MIS)
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_placed(sme, family, mis):
    """One workgroup, the generator's chunk origin, every misalignment."""
    c = T.corpus(family, mis)
    ctx, ix = _build_placed(sme, c, mis, 1)
    _counters(ctx, c)
    _check(ix, _ref(family, mis, 1, R), c)
    _markers(ix, c)


@pytest.mark.parametrize("mis", [0, 15])
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_placed_k2(sme, family, mis):
    """Bigrams: a token stored in the wrong slot of its record's token stream across
    an edge (tok_carry, dest_of) changes the record's bigrams, not its terms."""
    c = T.corpus(family, mis)
    ctx, ix = _build_placed(sme, c, mis, 2)
    _counters(ctx, c)
    _check(ix, _ref(family, mis, 2, R), c, K=2)


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_unplaced(sme, family):
    """Host bytes, default grid: every workgroup has its own chunk origin."""
    c = T.corpus(family, 0)
    ctx = sme.Context(1, R)
    ctx.load_docno_mapping(c.mapping())
    ix = ctx.build(c.bytes())
    _counters(ctx, c)
    _check(ix, _ref(family, 0, 1, R), c)
    _markers(ix, c)


# ---------------------------------------------------------------------------
# the neighbours
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense():
    c = T.dense_lt()
    return c, O.OracleIndex(c.bytes(), c.mapping(), 1, R)


@pytest.mark.parametrize("tok_grid", [0, 1])
def test_dense_lt(sme, tok_grid):
    """More '<' in one 16 KiB step of k_scan_lt than its LDS list holds: the rest
    go to the global list out of order.  6000 simple tags in a fast record, 4000
    complex ones in a slow one, and 20 KiB runs of '<' inside a record and
    between records."""
    c, ref = _dense()
    ctx, ix = _build_placed(sme, c, 0, 1, tok_grid)
    prof = _counters(ctx, c)
    print("lt_attempts", prof["lt_attempts"])
    _check(ix, ref, c)
    _markers(ix, c)


@functools.lru_cache(maxsize=None)
def _docwin():
    c = T.docid_window()
    return c, O.OracleIndex(c.bytes(), c.mapping(), 1, R)


@pytest.mark.parametrize("mis", [0, 9])
def test_docid_window(sme, mis):
    """<DOCNO> .. </DOCNO> on every side of byte 96 of k_docno's window, at every
    record start offset, ASCII and with a 2-byte character in the docid: every
    record gets its docno (the markers sit in the right document)."""
    c, ref = _docwin()
    ctx, ix = _build_placed(sme, c, mis, 1, 0)
    _counters(ctx, c)
    _check(ix, ref, c)
    _markers(ix, c)
