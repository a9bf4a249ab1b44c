"""The positions file on the device (sme_index_positions_file*, sme_index_attach_positions*):
the bytes an index with positions writes are the Python restatement's (posfile_ref,
from phrase_ref's streams); a file attached to an index without positions -- one
opened from its part files, one built without the option -- gives the streams back:
positions(), the file again, and every position feature's results bit for bit; every
width from the narrowest to 31 reads and writes; a merge carries attached streams;
and every malformed or foreign file is refused with its code and its place, the
index left as it was.  The encode / decode tile is 1024 positions
(csrc/sme_posfile.hpp kTile): the edges run T = 1023, 1024 and 1025.  Every comparison
is exact."""
import functools
import importlib
import struct

import numpy as np
import pytest

import ixdelete_cases as X
import load_streams as S
import phrase_ref as P
import posfile_ref as R
import test_gpu_ixdelete as D  # the corpora, _snapshot and the position features' query sets

pytestmark = pytest.mark.gpu

PKG = "simple-mapreduce-search-engine-information-retrieval-_amd"
SYN = importlib.import_module(PKG + ".synth")
SEQ = importlib.import_module(PKG + ".seqfile")
SME_EINVAL, SME_EPARSE, SME_ELIMIT = -1, -4, -6
TILE = 1024


# ---- corpora and their reference streams (computed once) ----------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus(name):
    """(corpus bytes, mapping bytes, phrase_ref stream records, [(docno, doc bytes)] or None)."""
    if name in ("fuzz", "synth"):
        docs, mb = D._corpus(name)
        c = D._bytes(docs)
    elif name == "c1":
        import test_gpu_phrase as PH
        (c, mb), docs = PH._corpus("c1"), None
    else:  # "need9": 288 terms, two tiles of positions
        assert name == "need9"
        c, mb, docs = SYN.gen_corpus(40, V=300, seed=5, len_lo=20, len_hi=60), SYN.mapping_bytes(40), None
    return c, mb, tuple(P.Streams(c, mb).records), docs


def _ref_file(ix, name, bits=0):
    return R.file_of(ix, list(_corpus(name)[2]), bits)


def _no_positions(sme, ix):
    assert ix.positions() == (0, 0, 0)
    D._raises(lambda: ix.query_phrase([[0]]), SME_EINVAL, "keeps no positions")


def _refused(sme, ix, data, code, *words, **kw):
    with pytest.raises(sme.SmeError) as e:
        ix.attach_positions(data, **kw)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    _no_positions(sme, ix)
    return str(e.value)


# ---- 1. file bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("name", ["fuzz", "synth"])
def test_file_bytes(sme, name, split):
    c, mb, recs, _ = _corpus(name)
    ix = D._ctx(sme, mb, 3, 1, positions=1, docid_split=split).build(c)
    want = _ref_file(ix, name)
    got = ix.positions_file()
    assert len(got) == len(want) and got == want
    st = ix.posfile_stats()
    assert (st["file_bytes"], st["bits"], st["checked_postings"]) == (len(want), R.need_bits(ix.V), 0)
    # the device entry: the same bytes, left in HBM
    ptr, n = ix.positions_file_device()
    host = np.zeros(n, np.uint8)
    sme.memcpy(host.ctypes.data, ptr, n)
    assert n == len(want) and host.tobytes() == want
    assert "encode" in ix.ctx.last_build_profile()


def test_file_bytes_c1(sme):
    c, mb, recs, _ = _corpus("c1")
    ix = D._ctx(sme, mb, 3, 0, positions=1).build(c)
    assert ix.positions_file() == _ref_file(ix, "c1")


# ---- 2. round trip through a directory -----------------------------------------------------------------
def _texts_and_sets(name):
    docs = _corpus(name)[3]
    dn = sorted(set(d for d, _ in docs))
    docsets = [dn[i:i + 7] for i in range(0, min(len(dn), 140), 7)] + [[0, -1, dn[0], dn[0]], []]
    return D._doc_texts(list(docs)), docsets


@pytest.mark.parametrize("idf_mode", [0, 1])
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("name", ["fuzz", "synth"])
def test_round_trip_through_directory(sme, tmp_path, name, R_, idf_mode):
    c, mb, recs, _ = _corpus(name)
    built = D._ctx(sme, mb, R_, idf_mode, positions=1).build(c)
    SEQ.write_index_dir(built, str(tmp_path), sync=b"\x07" * 16)
    assert SEQ.write_positions(built, str(tmp_path)).endswith("_positions")
    ctx = D._ctx(sme, mb, R_, idf_mode)
    loaded = SEQ.load_index_dir(ctx, str(tmp_path))  # the _positions file is no part
    _no_positions(sme, loaded)
    assert SEQ.attach_positions(loaded, str(tmp_path)) is loaded
    assert loaded.positions() == built.positions()
    assert loaded.positions_file() == built.positions_file() == _ref_file(built, name)
    texts, docsets = _texts_and_sets(name)
    D._same_position_features(loaded, built, texts, docsets)
    # and the forward index's own door
    fwd = sme.IntDocVectorsForwardIndex.from_dir(D._ctx(sme, mb, R_, idf_mode), str(tmp_path), positions=True)
    assert fwd.index.positions() == built.positions()
    assert sme.IntDocVectorsForwardIndex.from_dir(ctx, str(tmp_path)).index.positions() == (0, 0, 0)
    (tmp_path / "_positions").unlink()
    with pytest.raises(FileNotFoundError):
        sme.IntDocVectorsForwardIndex.from_dir(ctx, str(tmp_path), positions=True)


# ---- 3. attach to a build without the option ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["fuzz", "synth"])
def test_attach_to_plain_build(sme, name):
    c, mb, recs, _ = _corpus(name)
    built = D._ctx(sme, mb, 3, 1, positions=1).build(c)
    plain = D._ctx(sme, mb, 3, 1).build(c)
    before = D._snapshot(plain)
    assert before[4] == (0, 0, 0)
    data = built.positions_file()
    plain.attach_positions(data)
    after = D._snapshot(plain)
    assert after[:4] == before[:4] and after[4] == built.positions()  # nothing else moved
    assert D._term_records(plain) == D._term_records(built)
    st = plain.posfile_stats()
    assert plain.lookup([" "]).tolist() == [-1]  # the doc counter is no term of the vocabulary: none of P is its
    assert (st["file_bytes"], st["bits"], st["checked_postings"]) == (len(data), R.need_bits(plain.V), plain.P)
    prof = plain.ctx.last_build_profile()
    assert all(k in prof for k in ("digest", "decode", "crosscheck"))
    assert plain.positions_file() == data
    texts, docsets = _texts_and_sets(name)
    D._same_position_features(plain, built, texts, docsets)
    # through device memory, and without the cross-check
    other = D._ctx(sme, mb, 3, 1).build(c)
    ptr, n = built.positions_file_device()
    other.attach_positions_device(ptr, n, crosscheck=False)
    assert other.positions() == built.positions() and other.posfile_stats()["checked_postings"] == 0
    assert other.positions_file() == data


# ---- 4. every width ------------------------------------------------------------------------------------
CRAFTED = [(7, [0, 2, 2]), (9, [0, 0, 0]), (12, [0])]  # load_streams.VALID: apple 0 (9: 3, 7: 1, 12: 1), café€ 2 (7: 2)


def test_every_width_need_2(sme):
    ctx = sme.Context(1, 3)
    first = ctx.load_records(S.VALID)
    assert first.terms() == ["apple", "berry", "café€"] and R.need_bits(first.V) == 2
    dig = R.digest(first.terms())
    minimal = R.encode(CRAFTED, 3, dig)
    for b in range(2, 32):
        ix = ctx.load_records(S.VALID)
        ix.attach_positions(R.encode(CRAFTED, 3, dig, bits=b))
        assert ix.positions() == (3, 7, 8 * 4 + 4 * 7 + 4 * 3)
        assert ix.posfile_stats()["bits"] == b and ix.posfile_stats()["checked_postings"] == ix.P == 4
        assert ix.positions_file(bits=2) == minimal == ix.positions_file()
        assert ix.positions_file(bits=b) == R.encode(CRAFTED, 3, dig, bits=b)
    got = ix.query_phrase([[0, 2], [2, 2], [0, 0, 0], [0]])  # a loaded index answers phrases again
    assert got[0].tolist() == [0, 1, 2, 3, 6] and got[1].tolist() == [7, 7, 9, 7, 9, 12] and got[2].tolist() == [1, 1, 1, 1, 3, 1]
    for bad in (1, 32, -1):
        D._raises(lambda: ix.positions_file(bits=bad), SME_EINVAL, "bits")


def test_every_width_need_9(sme):
    c, mb, recs, _ = _corpus("need9")
    built = D._ctx(sme, mb, 2, 1, positions=1).build(c)
    assert R.need_bits(built.V) == 9 and built.positions()[1] > TILE
    minimal = _ref_file(built, "need9")
    assert built.positions_file() == minimal
    ctx = D._ctx(sme, mb, 2, 1)
    for b in range(9, 32):
        want = _ref_file(built, "need9", b)
        assert built.positions_file(bits=b) == want
        ix = ctx.build(c)
        ix.attach_positions(want)
        assert ix.posfile_stats()["bits"] == b
        assert ix.positions_file(bits=9) == minimal
    D._raises(lambda: built.positions_file(bits=8), SME_EINVAL, "bits 8")


# ---- 5. edges ---------------------------------------------------------------------------------------------
def _words(k):
    return " ".join("w%d" % (x % 7) for x in range(k))


EDGES = {
    "only_empty_records": [(None, ""), (None, "the of and")],
    "no_record": None,
    "one_record": [(3, "alpha beta alpha")],
    "empty_between": [("AMISSING", "kappa"), (None, ""), (5, "zed zed")],
    "longer_than_a_tile": [(2, _words(40)), (None, _words(TILE + 300)), (9, _words(3))],
}
for _k in (63, 64, 65, TILE - 1, TILE, TILE + 1):
    EDGES["T%d" % _k] = [(None, _words(_k))]


@pytest.mark.parametrize("case", sorted(EDGES))
def test_edges(sme, case):
    docs = EDGES[case]
    mb = D._edge_mapping()
    c = X.corpus_bytes(docs) if docs is not None else D.NO_RECORD
    recs = P.Streams(c, mb).records
    T = sum(len(s) for _, s in recs)
    if case.startswith("T"):
        assert T == int(case[1:])
    if case == "only_empty_records":
        assert T == 0 and len(recs) == 2
    if case == "empty_between":
        assert [len(s) for _, s in sorted(recs, key=lambda r: r[0])][1] == 0 and len(recs) == 3
    if case == "no_record":
        assert recs == []
    built = D._ctx(sme, mb, 2, 1, positions=1).build(c)
    assert built.positions()[:2] == (len(recs), T)
    want = R.file_of(built, recs)
    assert built.positions_file() == want
    h, back = R.decode(want)
    assert h["positions"] == T and back == R.streams_of(built, recs)
    plain = D._ctx(sme, mb, 2, 1).build(c)
    plain.attach_positions(want)
    assert plain.positions() == built.positions() and plain.positions_file() == want
    wide = D._ctx(sme, mb, 2, 1).build(c)
    wide.attach_positions(R.file_of(built, recs, 31))
    assert wide.positions_file() == want
    if T:
        ids = R.streams_of(built, recs)
        ph = [s[:2] for _, s in ids if len(s) >= 2][:4] + [s[-1:] for _, s in ids if s][:4]
        for order in (0, 1):
            D._same_result(plain.query_phrase(ph, order), built.query_phrase(ph, order), case)


# ---- 6. merge -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fuzz", "synth"])
def test_merge_carries_attached_streams(sme, tmp_path, name):
    c, mb, recs, docs = _corpus(name)
    half = len(docs) // 2
    a, b = D._bytes(docs[:half]), D._bytes(docs[half:])
    ctx = D._ctx(sme, mb, 3, 1, positions=1)
    whole = ctx.build(c)
    first = ctx.build(a)
    SEQ.write_index_dir(first, str(tmp_path), sync=b"\x05" * 16)
    SEQ.write_positions(first, str(tmp_path))
    second = ctx.build(b)
    loaded = SEQ.load_index_dir(ctx, str(tmp_path))
    assert ctx.merge([loaded, second]).positions() == (0, 0, 0)  # as before: one input without streams, none kept
    SEQ.attach_positions(loaded, str(tmp_path))
    merged = ctx.merge([loaded, second])
    assert merged.positions() == whole.positions()
    assert merged.positions_file() == whole.positions_file() == _ref_file(whole, name)
    phrases, _, _ = D._position_queries(D._token_ids(whole, D._doc_texts(list(docs))))
    for order in (0, 1):
        D._same_result(merged.query_phrase(phrases, order), whole.query_phrase(phrases, order), "phrase")


# ---- 7. refusals ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small():
    """Three documents of 70, 30 and 12 text words, the first two sharing words."""
    docs = [(11, " ".join("p%d" % (x % 5) for x in range(70))), (12, " ".join("p%d" % (x % 3) for x in range(30))),
            (20, " ".join("q%d" % (x % 4) for x in range(12)))]
    c = X.corpus_bytes(docs)
    return c, tuple(P.Streams(c, D._edge_mapping()).records)


def _small_index(sme, positions=0):
    return D._ctx(sme, D._edge_mapping(), 2, 1, positions=positions).build(_small()[0])


def _patch(data, at, fmt, value):
    out = bytearray(data)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def test_refused_headers(sme):
    ix = _small_index(sme)
    recs = list(_small()[1])
    good = R.file_of(ix, recs)
    h = R.sections(good)[0]
    N, T, V, need = ix.N, h["positions"], ix.V, R.need_bits(ix.V)
    assert (h["records"], h["V"], h["bits"]) == (N, V, need) and T > 66
    _refused(sme, ix, _patch(good, 7, "<B", 2), SME_EPARSE, "magic")
    _refused(sme, ix, _patch(good, 0, "<B", 0x54), SME_EPARSE, "magic")
    _refused(sme, ix, _patch(good, 8, "<I", 2), SME_EPARSE, "version 2")
    _refused(sme, ix, _patch(good, 8, "<I", 0), SME_EPARSE, "version 0")
    _refused(sme, ix, _patch(good, 12, "<I", need - 1), SME_EPARSE, "bits %d" % (need - 1))
    _refused(sme, ix, _patch(good, 12, "<I", 32), SME_EPARSE, "bits 32")
    _refused(sme, ix, _patch(good, 12, "<I", need + 1), SME_EPARSE, "size")  # a legal width, another length
    _refused(sme, ix, _patch(good, 16, "<Q", N + 1), SME_EPARSE, "records %d" % (N + 1))
    _refused(sme, ix, _patch(good, 16, "<Q", N - 1), SME_EPARSE, "records %d" % (N - 1))
    _refused(sme, ix, _patch(good, 32, "<Q", V + 1), SME_EPARSE, "V %d" % (V + 1))
    _refused(sme, ix, _patch(good, 32, "<Q", V - 1), SME_EPARSE, "V %d" % (V - 1))
    _refused(sme, ix, _patch(good, 24, "<Q", 1 << 31), SME_ELIMIT, "positions", "2^31")
    _refused(sme, ix, _patch(good, 24, "<Q", (1 << 31) - 1), SME_EPARSE, "size")
    for t in (T + 1, T - 1):  # the same byte count or another: the size, or the lengths' sum
        msg = _refused(sme, ix, _patch(good, 24, "<Q", t), SME_EPARSE)
        assert "size" in msg or ("len" in msg and str(t) in msg), msg
    _refused(sme, ix, _patch(good, 48, "<B", 1), SME_EPARSE, "reserved")
    _refused(sme, ix, _patch(good, 63, "<B", 0x80), SME_EPARSE, "reserved")
    _refused(sme, ix, good[:-1], SME_EPARSE, "size %d" % (len(good) - 1))
    _refused(sme, ix, good + b"\x00", SME_EPARSE, "size %d" % (len(good) + 1))
    _refused(sme, ix, good[:40], SME_EPARSE, "header")
    _refused(sme, ix, b"", SME_EPARSE, "header")
    _refused(sme, ix, _patch(good, 40, "<Q", (h["digest"] + 1) & R.M64), SME_EPARSE, "digest", "another vocabulary")
    terms = ix.terms()
    terms[0], terms[1] = terms[1], terms[0]
    _refused(sme, ix, _patch(good, 40, "<Q", R.digest(terms)), SME_EPARSE, "another vocabulary")
    # the untouched file is taken after all that
    ix.attach_positions(good)
    assert ix.positions()[:2] == (N, T)


def test_refused_structure(sme):
    ix = _small_index(sme)
    ids = R.streams_of(ix, list(_small()[1]))
    V, need, dig = ix.V, R.need_bits(ix.V), R.digest(ix.terms())
    flat = [t for _, s in ids for t in s]
    T = len(flat)
    assert T > 66 and V < (1 << (need + 1))

    def with_flat(new_flat, bits):
        out, p = [], 0
        for d, s in ids:
            out.append((d, new_flat[p:p + len(s)]))
            p += len(s)
        return R.encode(out, V, dig, bits)

    for b in (need + 1, 31):  # an id == V needs a width that holds it
        for p in (0, 63, 64, T - 1):
            bad = list(flat)
            bad[p] = V
            _refused(sme, ix, with_flat(bad, b), SME_EPARSE, "position %d " % p, "V = %d" % V)
        two = list(flat)
        two[64], two[5] = V, (1 << b) - 1
        _refused(sme, ix, with_flat(two, b), SME_EPARSE, "position 5 ")  # the first offence
    good = R.encode(ids, V, dig)
    h, d_at, l_at, w_at = R.sections(good)
    # a nonzero padding bit: the highest bit of the last word, and the first one past the last id
    assert (T * need) % 64 != 0
    _refused(sme, ix, _patch(good, len(good) - 1, "<B", good[-1] | 0x80), SME_EPARSE, "padding bits")
    last = len(good) - 8
    word = struct.unpack_from("<Q", good, last)[0] | (1 << ((T * need) % 64))
    _refused(sme, ix, _patch(good, last, "<Q", word), SME_EPARSE, "padding bits")
    assert ix.N % 2 == 1  # three records: four padding bytes after each section
    _refused(sme, ix, _patch(good, l_at - 4, "<I", 1), SME_EPARSE, "padding")
    _refused(sme, ix, _patch(good, w_at - 1, "<B", 1), SME_EPARSE, "padding")
    # a descending docno
    docnos = [d for d, _ in ids]
    assert docnos == sorted(docnos) and docnos[1] > -5
    _refused(sme, ix, _patch(good, d_at + 8, "<i", docnos[1] - 1), SME_EPARSE, "docno", "record 2 ")
    _refused(sme, ix, _patch(good, d_at, "<i", docnos[1] + 1), SME_EPARSE, "docno", "record 1 ")
    # the lengths one over and one under the header's positions
    ln = len(ids[1][1])
    _refused(sme, ix, _patch(good, l_at + 4, "<I", ln + 1), SME_EPARSE, "len", "add up to %d" % (T + 1))
    _refused(sme, ix, _patch(good, l_at + 4, "<I", ln - 1), SME_EPARSE, "len", "add up to %d" % (T - 1))
    _refused(sme, ix, _patch(good, l_at + 4, "<I", 0xFFFFFFFF), SME_EPARSE, "len")
    ix.attach_positions(good)
    assert ix.positions()[:2] == (ix.N, T)


def test_crosscheck(sme):
    ids = None
    for crosscheck in (True, False):
        ix = _small_index(sme)
        ids = R.streams_of(ix, list(_small()[1]))
        V, dig = ix.V, R.digest(ix.terms())
        # one position's id replaced by another valid id
        (d0, s0), (d1, s1) = ids[0], ids[1]
        t1, t2 = s0[3], next(t for t in range(V) if t != s0[3])
        swapped = [(d0, s0[:3] + [t2] + s0[4:])] + ids[1:]
        # one position moved from the end of a record to the start of the next: the structure still holds
        moved = [(d0, s0[:-1]), (d1, s0[-1:] + s1)] + ids[2:]
        assert d0 < d1
        for bad, words in ((swapped, ("term %d " % min(t1, t2), "docno %d" % d0)),
                           (moved, ("term %d " % s0[-1], "docno %d" % d0))):
            data = R.encode(bad, V, dig)
            if crosscheck:
                _refused(sme, ix, data, SME_EPARSE, "cross-check", *words)
            else:  # what the flag gives up: a file of the right structure and the wrong content is taken
                other = _small_index(sme)
                other.attach_positions(data, crosscheck=False)
                assert other.positions()[:2] == (len(bad), sum(len(s) for _, s in bad))
                assert other.posfile_stats()["checked_postings"] == 0
                assert R.decode(other.positions_file())[1] == bad
        ix.attach_positions(R.encode(ids, V, dig), crosscheck=crosscheck)
        assert ix.posfile_stats()["checked_postings"] == (ix.P if crosscheck else 0)


def test_refused_calls(sme):
    c = _small()[0]
    built = _small_index(sme, positions=1)
    data = built.positions_file()
    ix = _small_index(sme)
    D._raises(lambda: ix.positions_file(), SME_EINVAL, "keeps no positions")
    ix.attach_positions(data)
    before = ix.positions()
    D._raises(lambda: ix.attach_positions(data), SME_EINVAL, "already keeps positions")  # attaching twice
    D._raises(lambda: built.attach_positions(data), SME_EINVAL, "already keeps positions")
    assert ix.positions() == before and ix.positions_file() == data
    k2 = sme.Context(2, 2)
    k2.load_docno_mapping(D._edge_mapping())
    ix2 = k2.build(c)
    D._raises(lambda: ix2.attach_positions(data), SME_EINVAL, "K != 1")
    D._raises(lambda: ix2.positions_file(), SME_EINVAL, "K != 1")
    cg = sme.Context(2, 2).build_chargram(c)
    D._raises(lambda: sme.Index.attach_positions(cg, data), SME_EINVAL, "not a TermKGramDocIndexer index")
    D._raises(lambda: sme.Index.positions_file(cg), SME_EINVAL, "not a TermKGramDocIndexer index")
    fresh = _small_index(sme)
    rc = sme.lib().sme_index_attach_positions(fresh._h, data, len(data), 2, None)
    assert rc == SME_EINVAL and b"flag" in sme.lib().sme_last_error()
    rc = sme.lib().sme_index_attach_positions(fresh._h, None, 0, 0, None)
    assert rc == SME_EINVAL and b"null" in sme.lib().sme_last_error()
    _no_positions(sme, fresh)
    # a file of another index: same shape of header, other documents
    other = D._ctx(sme, D._edge_mapping(), 2, 1, positions=1).build(X.corpus_bytes([(11, "p0 p1"), (12, "p2"), (20, "q0")]))
    _refused(sme, fresh, other.positions_file(), SME_EPARSE)
