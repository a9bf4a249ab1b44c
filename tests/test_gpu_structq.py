"""Structured queries on the device (sme_query_structured*): Boolean groups whose
members are leaves -- a term, or an ordered / unordered window over terms.  Every
offset, docno and score is held to structq_ref.py, the composition of near_ref and
bool_ref (pinned by test_structq_ref.py): offsets and docnos exactly, scores bit
for bit.  Where code exists that answers the same question -- a term-only batch is
sme_query_boolean, a single operator leaf is sme_query_near -- the answers are held
to that code too.  No tolerance anywhere."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import near_ref as NR
import oracle_lib as O
import phrase_ref as P
import structq_ref as SR
import test_gpu_near as TN  # (their corpora and helpers; nothing of them is changed)
import test_gpu_phrase as TP

pytestmark = pytest.mark.gpu

SME_EINVAL, SME_ELIMIT = -1, -6
ORDERS = ((0, 0), (1, 0), (1, 3), (0, 1))
_ctx, _raises, _doc = TP._ctx, TP._raises, TP._doc
REQ, EXC = False, True


def T(t):
    return ([int(t)], 0, 0)


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]), np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:8]
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:8]
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64)), np.nonzero(got[2] != want[2])[0][:8]


def _ref(ix, st, queries, order=0, m=0, idf_mode=0, N=None, first_driver=False):
    terms = ix.terms()
    return SR.run(st, ix.weights(), queries, order, m, idf_mode, N, terms.__getitem__, first_driver)


def _tid(ix, word):
    return int(ix.lookup(O.process_content(word))[0])


def _leaf(q):
    """near's (ids, width, ordered) as a leaf."""
    return (list(q[0]), 1 if q[2] else 2, q[1])


# ---- 1. reference parity, 3. narrowing on the same batch ---------------------------
SHAPES = ("alone", "and_term", "and_rare", "or_first", "or_second", "excluded")


def _shaped(near_ids, fill, a):
    """Every proximity query in each shape; -> (queries, shape of each)."""
    qs, shape = [], []
    for q in near_ids:
        p = _leaf(q)
        for name, groups in (("alone", [([p], REQ)]),
                             ("and_term", [([p], REQ), ([T(fill)], REQ)]),
                             ("and_rare", [([T(a)], REQ), ([p], REQ)]),
                             ("or_first", [([p, T(a)], REQ)]),
                             ("or_second", [([T(a), p], REQ)]),
                             ("excluded", [([T(fill)], REQ), ([p], EXC)])):
            qs.append(groups)
            shape.append(name)
    return qs, shape


@pytest.mark.parametrize("idf_mode", [0, 1])
def test_reference_parity_and_narrowing(sme, idf_mode):
    corpus, mapping, _, _ = TN._edge()
    st, near_q, _ = TN._edge_ref()
    ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
    fill, a = _tid(ix, TN.FILL), _tid(ix, TN.A)
    queries, shape = _shaped(TN._q(ix, near_q), fill, a)
    nops = len(near_q) * len(SHAPES)
    want = {key: _ref(ix, st, queries, key[0], key[1], idf_mode) for key in ORDERS}
    # before any device comparison: the reference's own answer reaches every shape
    off = want[0, 0][0][0]
    for name in SHAPES:
        assert any(off[i + 1] > off[i] for i, s in enumerate(shape) if s == name), name
    # ... and the excluded leaf removes something somewhere
    plain = _ref(ix, st, [[([T(fill)], REQ)]], 0, 0, idf_mode)[0][0][1]
    assert any(0 < off[i + 1] - off[i] < plain for i, s in enumerate(shape) if s == "excluded")
    verified = {}
    try:
        for narrow in (1, 0):
            ix.ctx.set_option("struct_narrow", narrow)
            for key in ORDERS:
                res, cands, total, lists = want[key]
                _same(ix.query_structured(queries, *key), res)
                leaves, ver, c, mt = ix.structured_stats()
                assert (leaves, mt) == (nops, total) and ver > 0
                if narrow == 0 or idf_mode == 1:  # whole leaves: the reference's drivers are the device's
                    assert c == cands
            verified[narrow] = ix.structured_stats()[1]
    finally:
        ix.ctx.set_option("struct_narrow", 1)
    if idf_mode == 0:
        assert verified[1] < verified[0]
    else:  # the true-df mode evaluates leaves whole whatever the option says
        assert verified[1] == verified[0]
    # the leaves evaluated whole are sme_query_near's own work, once per leaf
    ix.query_near([q for q in TN._q(ix, near_q) for _ in SHAPES])
    assert ix.near_stats()[1] == verified[0]


# ---- the crafted corpus of 2 (facade), 3 (narrowing) and 4 (chunks, drivers) -------
SIZES = {63: "alfa", 64: "bravo", 65: "delta", 129: "echo"}  # (the stemmer leaves them alone)
NCRAFT = 200


@functools.lru_cache(maxsize=None)
def _craft():
    """200 one-record documents, docno d = 1 .. 200.  The filler phrase "kilo lima" is
    in all of them; "<tag> kilo" in the first n for n = 63, 64, 65, 129; quebec in
    exactly d = 7 and 99; mike in every 5th; "nova zulu oscar" in every 10th;
    zulfiqar in every 3rd beside zulu in all."""
    docs, ids = [], []
    for d in range(1, NCRAFT + 1):
        parts = []
        for n, tag in SIZES.items():
            if d <= n:
                parts += [tag, "kilo"]
        parts += ["kilo", "lima", "zulu"]
        if d in (7, 99):
            parts.append("quebec")
        if d % 5 == 0:
            parts.append("mike")
        if d % 10 == 0:
            parts += ["nova", "zulu", "oscar"]
        if d % 3 == 0:
            parts.append("zulfiqar")
        ids.append("CR%06d-%02d" % (d, d % 100))
        docs.append(_doc(ids[-1], " ".join(parts)))
    corpus = "".join(docs).encode("utf-8")
    mapping = O.write_mapping(ids)
    return corpus, mapping, P.Streams(corpus, mapping)


def _words(ix, *words):
    return [_tid(ix, w) for w in words]


def test_narrowing_counts(sme):
    corpus, mapping, st = _craft()
    for idf_mode in (0, 1):
        ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
        kilo, lima, quebec = _words(ix, "kilo", "lima", "quebec")
        assert int(np.diff(ix.offsets())[quebec]) == 2
        phrase = ([kilo, lima], 1, 1)
        ix.query_near([([kilo, lima], 1, True)])
        full = ix.near_stats()[1]
        assert full == ix.near_stats()[2] == NCRAFT >= 130
        queries = [[([phrase], REQ), ([T(quebec)], REQ)]]
        res = _ref(ix, st, queries, 1, 0, idf_mode)[0]
        assert res[1].tolist() == [7, 99]
        got = {}
        try:
            for narrow in (1, 0):
                ix.ctx.set_option("struct_narrow", narrow)
                _same(ix.query_structured(queries, 1, 0), res)
                got[narrow] = ix.structured_stats()
        finally:
            ix.ctx.set_option("struct_narrow", 1)
        assert got[0] == (1, full, 2, 2)
        assert got[1] == ((1, 2, 2, 2) if idf_mode == 0 else (1, full, 2, 2))
        if idf_mode == 0:
            # an excluded leaf and a leaf in an OR group beside term-only groups are narrowed as well
            queries = [[([T(quebec)], REQ), ([phrase], EXC)], [([phrase, T(kilo)], REQ), ([T(quebec)], REQ)],
                       [([T(quebec), T(-1)], REQ), ([T(kilo)], REQ), ([phrase], REQ)]]
            _same(ix.query_structured(queries), _ref(ix, st, queries)[0])
            assert ix.structured_stats()[:2] == (3, 6)
            # a required term group without a posting: nothing can match, nothing is verified
            queries = [[([phrase], REQ), ([T(-1)], REQ)], [([phrase], REQ), ([], REQ)]]
            got = ix.query_structured(queries)
            assert got[0].tolist() == [0, 0, 0] and ix.structured_stats() == (2, 0, 0, 0)


# ---- 2. equivalences ---------------------------------------------------------------
def _term_batch(ix, seed, nq=40):
    """Random Boolean queries, mostly over the index's most frequent terms (so that they match)."""
    rng = random.Random(seed)
    top = np.argsort(-np.diff(ix.offsets()), kind="stable")[:8].tolist()
    qs = []
    for _ in range(nq):
        groups = []
        for _ in range(rng.randint(0, 4)):
            ids = [rng.choice(top + [-1, rng.randrange(ix.V)]) for _ in range(rng.randint(0, 3))]
            groups.append((ids, rng.random() < 0.25))
        qs.append(groups)
    return qs


def test_term_only_batch_is_query_boolean(sme):
    corpus, mapping, _, _ = TP._driver()
    plain = _ctx(sme, mapping, 1, 0, positions=0).build(corpus)
    ctx2 = _ctx(sme, mapping, 1, 0, positions=0, R=2)
    indexes = {"positions": _ctx(sme, mapping, 1, 1).build(corpus), "plain": plain,
               "k2": _ctx(sme, mapping, 2, 0).build(corpus),
               "loaded": ctx2.load_records([bytes(plain.partition_records(p)) for p in range(2)])}
    for name, ix in indexes.items():
        bq = _term_batch(ix, 5)
        sq = [[([T(t) for t in ids], ex) for ids, ex in groups] for groups in bq]
        hits = 0
        for order, m in ORDERS:
            want = ix.query_boolean(bq, order, m)
            _same(ix.query_structured(sq, order, m), want)
            assert ix.structured_stats() == (0, 0) + ix.boolean_stats()
            hits = max(hits, int(want[0][-1]))
        assert hits > 50, name
        if name != "positions":  # a batch with one operator leaf anywhere is refused, in sme_query_near's words
            mixed = sq + [[([([0], 1, 1)], REQ)]]
            for entry in (ix.query_structured, ix.query_structured_device):
                _raises(lambda: entry(mixed), SME_EINVAL, "K" if name == "k2" else "positions")
            _same(ix.query_structured(sq), ix.query_boolean(bq))  # and the index stays usable


@pytest.mark.parametrize("idf_mode", [0, 1])
def test_single_operator_leaf_is_query_near(sme, idf_mode):
    corpus, mapping, _, _ = TP._driver()
    ix = _ctx(sme, mapping, 1, idf_mode).build(corpus)
    ids = TN._q(ix, TN._driver_queries())
    sq = [[([_leaf(q)], REQ)] for q in ids]
    for order, m in ORDERS:
        off, dn, _, sc = ix.query_near(ids, order, m)
        _same(ix.query_structured(sq, order, m), (off, dn, sc))
        assert off[-1] > 10
    near = ix.near_stats()
    assert ix.structured_stats() == (len(ids), near[1], near[2], near[2])
    # an ordered leaf of one term, whatever its width, is the term leaf
    ts = [_tid(ix, w) for w in ("kilo", "lima", TP.RARE[63], TP.RARE[257])]
    want = ix.query_structured([[([T(t)], REQ)] for t in ts], 1, 0)
    assert want[0][-1] > 300
    for width in (1, 4, 2 ** 31 - 1):
        _same(ix.query_structured([[([([t], 1, width)], REQ)] for t in ts], 1, 0), want)


# ---- 4. chunk and driver edges -----------------------------------------------------
def test_chunk_and_driver_edges(sme):
    corpus, mapping, st = _craft()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    kilo, lima, zulu = _words(ix, "kilo", "lima", "zulu")
    queries, sizes = [], []
    for n, tag in SIZES.items():
        t = _tid(ix, tag)
        ph = ([t, kilo], 1, 1)
        # the operator leaf drives (n entries against lima's 200); it drives as the
        # first group; the driver is an OR of a term and a leaf that share documents
        queries += [[([T(lima)], REQ), ([ph], REQ)], [([ph], REQ), ([T(zulu)], REQ)], [([T(t), ph], REQ)],
                    [([ph, T(t)], REQ), ([T(lima)], REQ)], [([ph, ([kilo, lima], 2, 5)], REQ), ([T(t)], EXC)]]
        sizes.append(n)
    want = {(o, m, f): _ref(ix, st, queries, o, m, 0, first_driver=bool(f))
            for o, m in ((0, 0), (1, 7)) for f in (0, 1)}
    lists = want[0, 0, 0][3]
    assert np.diff(lists[0])[0::6][:4].tolist() == sizes == [63, 64, 65, 129]  # the virtual lists' sizes
    off, dn = want[0, 0, 0][0][0], want[0, 0, 0][0][1]
    for i, n in enumerate(sizes):
        assert np.diff(off)[5 * i:5 * i + 5].tolist() == [n, n, n, n, NCRAFT - n]
        for j in (2, 3):  # shared documents come out once
            one = dn[off[5 * i + j]:off[5 * i + j + 1]]
            assert len(set(one.tolist())) == len(one) == n
    try:
        ix.ctx.set_option("struct_narrow", 0)  # whole leaves: the driver entries are the reference's
        for chunk in (64, 1024, 4096):
            ix.ctx.set_option("bool_chunk", chunk)
            for drv in (0, 1):
                ix.ctx.set_option("bool_driver", drv)
                for o, m in ((0, 0), (1, 7)):
                    res, cands, total, _ = want[o, m, drv]
                    _same(ix.query_structured(queries, o, m), res)
                    assert ix.structured_stats()[2:] == (cands, total)
        ix.ctx.set_option("struct_narrow", 1)
        ix.ctx.set_option("bool_driver", 0)
        for chunk in (64, 4096):
            ix.ctx.set_option("bool_chunk", chunk)
            _same(ix.query_structured(queries, 1, 7), want[1, 7, 0][0])
    finally:
        for name, v in (("bool_chunk", 1024), ("bool_driver", 0), ("struct_narrow", 1)):
            ix.ctx.set_option(name, v)
    # the leaf drives: one query alone examines exactly its n entries
    for i, n in enumerate(sizes):
        ix.query_structured([queries[5 * i]])
        assert ix.structured_stats()[2] == n


# ---- 5. independent buffers, the device entry, degenerate batches ---------------------
def test_device_entry_and_independent_buffers(sme):
    corpus, mapping, st = _craft()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    kilo, lima, mike, zulu = _words(ix, "kilo", "lima", "mike", "zulu")
    queries = [[([([kilo, lima], 1, 1)], REQ), ([T(mike)], REQ)], [], [([T(zulu), ([mike, kilo], 2, 9)], REQ)],
               [([([kilo, lima], 1, 1)], EXC)], [([T(mike)], REQ), ([([lima, zulu], 1, 2)], EXC)]]
    host = ix.query_structured(queries, 1, 9)
    _same(host, _ref(ix, st, queries, 1, 9)[0])
    assert host[0].tolist() == [0, 9, 9, 18, 18, 18]
    bq = [[([kilo], False), ([mike], False)]]
    b = ix.query_boolean(bq, 1, 5)
    p = ix.query_phrase([[kilo, lima]], 0, 6)
    n = ix.query_near([([lima, kilo], 4, False)], 1, 7)
    d_b = ix.query_boolean_device(bq, 1, 5)
    d_p = ix.query_phrase_device([[kilo, lima]], 0, 6)
    d_n = ix.query_near_device([([lima, kilo], 4, False)], 1, 7)
    d_off, d_dn, d_sc, total = ix.query_structured_device(queries, 1, 9)  # between them: their arrays stay
    ix.expand_wildcards(["k*"])

    def fetch(ptr, count, dt):
        a = np.zeros(count, dt)
        sme.memcpy(a.ctypes.data, ptr, a.nbytes)
        return a

    assert total == host[0][-1] == 18
    _same((fetch(d_off, len(queries) + 1, np.int64), fetch(d_dn, total, np.int32), fetch(d_sc, total, np.float64)), host)
    assert np.array_equal(fetch(d_b[1], d_b[3], np.int32), b[1]) and len(b[1]) == 5
    assert fetch(d_b[2], d_b[3], np.float64).tobytes() == b[2].tobytes()
    assert np.array_equal(fetch(d_p[1], d_p[4], np.int32), p[1]) and len(p[1]) == 6
    assert np.array_equal(fetch(d_n[1], d_n[4], np.int32), n[1]) and len(n[1]) == 7
    assert fetch(d_n[3], d_n[4], np.float64).tobytes() == n[3].tobytes()
    # and the other way round
    ix.query_boolean(bq)
    ix.query_phrase([[lima, zulu]])
    ix.query_near([([kilo], 1, True)])
    assert np.array_equal(fetch(d_dn, total, np.int32), host[1])
    assert fetch(d_sc, total, np.float64).tobytes() == host[2].tobytes()
    # nq == 0; a batch of empty and purely negative queries
    for entry in (ix.query_structured, ix.query_structured_device):
        entry([], 1, 5)
        assert ix.structured_stats() == (0, 0, 0, 0)
    got = ix.query_structured([])
    assert got[0].tolist() == [0] and got[1].size == got[2].size == 0
    none = [[], [([([kilo, lima], 1, 1)], EXC)], [([T(kilo)], EXC), ([T(mike), ([kilo], 2, 1)], EXC)], [([], EXC)], []]
    got = ix.query_structured(none, 1, 3)
    assert got[0].tolist() == [0] * 6 and got[1].size == 0
    assert ix.structured_stats()[0] == 2 and ix.structured_stats()[2:] == (0, 0)
    assert ix.query_structured_device(none)[3] == 0


def test_host_arrays_live_until_the_features_next_call(sme):
    """include/sme.h's promise for the host entries, seen through the C ABI itself (the
    Python wrappers copy at once): the arrays one feature's host entry hands out stay
    as they are while the other five features' host entries and all six device
    entries run; a batch without a result still hands out valid column pointers; and
    the feature answers its first batch again after that."""
    corpus, mapping, _ = _craft()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    L = sme.lib()
    kilo, lima, mike, zulu = _words(ix, "kilo", "lima", "mike", "zulu")
    i32, i64, u8, f64 = C.c_int32, C.c_int64, C.c_uint8, C.c_double
    CT = {np.int32: i32, np.int64: i64, np.uint8: u8}

    def typed(arrays, dtypes):  # (one element behind an empty array, as the wrappers keep)
        keep = [np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt) for a, dt in zip(arrays, dtypes)]
        return keep, [a.ctypes.data_as(C.POINTER(CT[dt])) for a, dt in zip(keep, dtypes)]

    def text(words, *more):
        bs = [w.encode() for w in words]
        offs = np.cumsum([0] + [len(b) for b in bs]).astype(np.int64)
        return offs, [b"".join(bs), offs.ctypes.data_as(C.POINTER(i64)), len(bs), *more], len(bs)

    def ids(arrays, dtypes, nq_at, order, m):
        keep, ptrs = typed(arrays, dtypes)
        nq = len(arrays[nq_at]) - 1
        return keep, ptrs + [nq, order, m], nq

    I = sme.Index
    phrase = ([kilo, lima], 1, 1)
    # feature: (host entry, device entry, column ctypes, arguments of a batch, first / other / empty batch)
    features = {
        "wx": (L.sme_index_expand_wildcards, L.sme_index_expand_wildcards_device, (i32,), lambda b: text(b),
               ["k*", "zul*"], ["m*", "*a"], ["xyzzy*", "q?q"]),
        "fz": (L.sme_index_suggest_terms, L.sme_index_suggest_terms_device, (i32, u8), lambda b: text(b, 1, 10),
               ["kilo", "limo", "zulo"], ["mikes"], ["qqqqqqqqqq", "xxxxxxxx"]),
        "bq": (L.sme_query_boolean, L.sme_query_boolean_device, (i32, f64),
               lambda b: ids(I.boolean_arrays(b), (np.int32, np.int64, np.uint8, np.int64), 3, 1, 5),
               [[([kilo], False), ([mike], False)], [([zulu], False)]], [[([lima], False)]], [[([-1], False)], []]),
        "pq": (L.sme_query_phrase, L.sme_query_phrase_device, (i32, i32, f64),
               lambda b: ids(I.phrase_arrays(b), (np.int32, np.int64), 1, 0, 6),
               [[kilo, lima], [lima, zulu]], [[zulu, mike]], [[-1, kilo], [lima, kilo]]),
        "nq": (L.sme_query_near, L.sme_query_near_device, (i32, i32, f64),
               lambda b: ids(I.near_arrays(b), (np.int32, np.int64, np.int32, np.uint8), 1, 1, 7),
               [([lima, kilo], 4, False), ([kilo, lima], 1, True)], [([kilo], 1, True)], [([-1, kilo], 2, True)]),
        "sq": (L.sme_query_structured, L.sme_query_structured_device, (i32, f64),
               lambda b: ids(I.structured_arrays(b),
                             (np.int32, np.int64, np.uint8, np.int32, np.int64, np.uint8, np.int64), 6, 1, 9),
               [[([phrase], REQ), ([T(mike)], REQ)], [([T(zulu), ([mike, kilo], 2, 9)], REQ)]],
               [[([T(lima)], REQ)]], [[([T(-1)], REQ)], [([phrase], REQ), ([T(-1)], REQ)]]),
    }

    def host(name, batch):
        """-> (queries, the raw pointers handed out: offsets, then every column)"""
        entry, _, cols, args, *_ = features[name]
        keep, a, n = args(batch)
        outs = [C.POINTER(ct)() for ct in (i64,) + cols]
        assert entry(ix._h, *a, *[C.byref(o) for o in outs]) == 0, L.sme_last_error()
        return n, outs

    def device(name, batch):
        _, entry, cols, args, *_ = features[name]
        keep, a, n = args(batch)
        outs, tot = [C.c_void_p() for _ in range(len(cols) + 1)], i64()
        assert entry(ix._h, *a, None, *[C.byref(o) for o in outs], C.byref(tot)) == 0, L.sme_last_error()

    def read(n, outs):
        """what the pointers point at now, as bytes: offsets[n + 1], then every column[total]"""
        off = np.ctypeslib.as_array(outs[0], (n + 1,))
        total = int(off[n])
        return [off.tobytes()] + [np.ctypeslib.as_array(o, (total,)).tobytes() if total else b"" for o in outs[1:]]

    for name, (_, _, cols, _, first, other, empty) in features.items():
        n, outs = host(name, first)
        copy = read(n, outs)
        assert all(len(c) > 0 for c in copy[1:]) and len(copy) == len(cols) + 1, name  # the batch has results
        for o in features:
            if o != name:
                host(o, features[o][5])
        for o in features:
            device(o, features[o][5])
        assert read(n, outs) == copy, name
        # a batch with queries and no result: valid pointers, every offset 0
        ne, eouts = host(name, empty)
        assert all(bool(p) for p in eouts), name
        assert np.ctypeslib.as_array(eouts[0], (ne + 1,)).tolist() == [0] * (ne + 1), name
        # ... after which the arrays serve the first batch again
        assert read(*host(name, first)) == copy, name


# ---- 6. refusals ---------------------------------------------------------------------
def test_refusals(sme):
    corpus, mapping, _ = _craft()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    t = _tid(ix, "kilo")
    ok = [([T(t)], REQ)]
    ph = ([t, t], 1, 1)
    one = ix.query_structured([ok, [([ph], REQ)]])
    for entry in (ix.query_structured, ix.query_structured_device):
        # at the limits: accepted
        entry([[([T(t)], REQ)] * 64, [([T(t)] * 1024, REQ)], [([([t] * 32, 2, 2 ** 31 - 1)], REQ)]], 0, 1)
        _raises(lambda: entry([ok, [([T(t)], REQ)] * 65]), SME_ELIMIT, "query 1")
        _raises(lambda: entry([[([T(t)] * 1025, REQ)]]), SME_ELIMIT, "query 0")
        _raises(lambda: entry([ok, ok, [([([t] * 33, 1, 1)], REQ)]]), SME_ELIMIT, "query 2")
        _raises(lambda: entry([ok, [([([t, t], 0, 0)], REQ)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([[([([], 0, 0)], REQ)]]), SME_EINVAL, "query 0")
        _raises(lambda: entry([ok, [([([t], 3, 1)], REQ)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([[([([t, t], 1, 0)], REQ)]]), SME_EINVAL, "query 0")
        _raises(lambda: entry([ok, [([([t, t], 2, -4)], EXC)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([ok, [([T(ix.V)], REQ)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([[([([t, -2], 1, 1)], REQ)]]), SME_EINVAL, "query 0")
        _raises(lambda: entry([ok, [([T(t)], 2)]]), SME_EINVAL, "query 1")
        _raises(lambda: entry([ok], 2, 0), SME_EINVAL, "order")
        _raises(lambda: entry([ok], 0, -1), SME_EINVAL, "m must")
        # offsets that do not ascend from 0, at each level (the C ABI takes no array sizes: a
        # level cut short against the one above is tools/structq_check.cc's ground)
        a = list(sme.Index.structured_arrays([ok, [([ph, T(t)], EXC)]]))
        entry(None, arrays=a)
        for k, bad, word in ((6, [0, 2, 1], "query 1"), (6, [1, 1, 2], None), (4, [0, 2, 1], "query 1"),
                             (4, [1, 1, 3], None), (1, [0, 1, 3, 2], "query 1"), (1, [1, 1, 3, 4], None),
                             (1, [0, 2, 1, 4], "query 1")):
            b = list(a)
            b[k] = np.array(bad, np.int64)
            _raises(lambda: entry(None, arrays=b), SME_EINVAL, word)
    # a NULL array where the batch has entries of that level
    L = sme.lib()
    q = np.array([0, 1], np.int64)
    ro, dn, sc = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
    i64p = C.POINTER(C.c_int64)
    rc = L.sme_query_structured(ix._h, None, q.ctypes.data_as(i64p), None, None, q.ctypes.data_as(i64p), None,
                                q.ctypes.data_as(i64p), 1, 0, 0, C.byref(ro), C.byref(dn), C.byref(sc))
    assert rc == SME_EINVAL
    rc = L.sme_query_structured(ix._h, None, None, None, None, None, None, q.ctypes.data_as(i64p), 1, 0, 0,
                                C.byref(ro), C.byref(dn), C.byref(sc))
    assert rc == SME_EINVAL
    cg = sme.Context(2, 2)
    out = cg.build_chargram(corpus)
    rc = L.sme_query_structured(out._h, None, None, None, None, None, None, None, 0, 0, 0, C.byref(ro), C.byref(dn),
                                C.byref(sc))
    assert rc == SME_EINVAL and b"TermKGramDocIndexer" in L.sme_last_error()
    _same(ix.query_structured([ok, [([ph], REQ)]]), one)  # an error leaves the index usable


# ---- 7. reweight ---------------------------------------------------------------------
def test_reweight(sme):
    corpus, mapping, st = _craft()
    ix = _ctx(sme, mapping, 1, 1).build(corpus)
    kilo, lima, mike, nova, oscar = _words(ix, "kilo", "lima", "mike", "nova", "oscar")
    queries = [[([([kilo, lima], 1, 1)], REQ), ([T(mike)], REQ)], [([([nova, oscar], 2, 3), T(mike)], REQ)],
               [([T(mike)], REQ), ([([nova, oscar], 1, 2)], EXC)]]
    before = ix.query_structured(queries, 1, 0)
    _same(before, _ref(ix, st, queries, 1, 0, 1)[0])
    ix.reweight(3 * ix.N)
    after = ix.query_structured(queries, 1, 0)
    _same(after, _ref(ix, st, queries, 1, 0, 1, N=3 * ix.N)[0])
    assert np.array_equal(before[0], after[0]) and before[0][-1] > 50
    assert not np.array_equal(np.sort(before[2]), np.sort(after[2]))
    ix.reweight(ix.N)
    _same(ix.query_structured(queries, 1, 0), before)


# ---- 8. the facade -------------------------------------------------------------------
def test_facade(sme):
    corpus, mapping, st = _craft()
    ix = _ctx(sme, mapping, 1, 0).build(corpus)
    fw = sme.IntDocVectorsForwardIndex(ix, mapping)
    kilo, lima, mike, nova, oscar = _words(ix, "kilo", "lima", "mike", "nova", "oscar")
    _, zs = ix.expand_wildcards(["zul*"])
    assert len(zs) >= 2
    want = [([([kilo, lima], 1, 1)], False), ([T(mike)], False), ([([nova, oscar], 2, 3)], True),
            ([T(z) for z in zs], False)]
    assert fw.get_structured('"kilo lima" mike -#uw:3(nova oscar) zul*') == want
    res = _ref(ix, st, [want], 1, 10)[0]
    assert fw.rank_structured(10) == res[1].tolist() and len(res[1]) == 10
    assert all(d % 5 == 0 and d % 10 != 0 for d in res[1].tolist())
    # stop words are dropped as get_boolean drops them; an unknown word is -1; an OR group of words
    assert fw.get_structured("the Mike of") == [([T(mike)], False)]
    assert fw.get_structured("mike -xylophone") == [([T(mike)], False), ([T(-1)], True)]
    assert fw.rank_structured(3) == _ref(ix, st, [[([T(mike)], REQ)]], 1, 3)[0][1].tolist()
    assert fw.get_structured('nova|"the kilo of lima"|the') == [([T(nova), ([kilo, lima], 1, 1)], False)]
    assert fw.rank_structured(4) == _ref(ix, st, [[([T(nova), ([kilo, lima], 1, 1)], REQ)]], 1, 4)[0][1].tolist()
    assert fw.get_structured("the|of") == [] and fw.rank_structured() == []
    assert fw.get_structured('"kilo xylophone"')[0][0][0][0] == [kilo, -1] and fw.rank_structured() == []
    with pytest.raises(ValueError):
        fw.get_structured('"kilo lima')
