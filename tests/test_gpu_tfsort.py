"""The tf-desc segment sort (csrc/sme_tfsort.hip: tf_sort_segments) against numpy,
bit-exact: per segment of a CSR, np.argsort(-tf, kind="stable") applied to docno
and tf.  Through libsme_prims.so (tests/native/prims_tfsort.hip) with the guard
and fill discipline of the other primitive tests: both inputs must come back
unchanged, and nothing may be written past an output or a scratch buffer.

Segment lengths sit on every class boundary (tiny <= 8, small <= 64, wave <= 512,
medium <= 8192, large: tiles of 4096) and on the kernels' batch boundaries: a wave
keeps K = 8 chunks of 64 postings in flight (512 per wave, 2048 per 4-wave
workgroup), the tile count 4 x 64 16-byte loads (1024 postings).  Neighbours are
of different classes with empty segments between them, so an overrun lands in
a checked neighbour or a guard, and large segments start at every offset modulo
16 bytes (the tile count reads 16 bytes at a time).  The tiles' counters are
ordered by one device-wide scan; the many-large CSR makes that scan span several
of its own tiles and a hundred segments."""
import ctypes as C

import numpy as np
import pytest

import prims_lib as PL

pytestmark = pytest.mark.gpu

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
GUARDS = ("off", "docno_d", "tf_d", "docno_o", "tf_o", "lists", "tiles", "tcnt", "scan", "nseg",
          "an input's contents", "a scratch buffer outgrew its documented size")
K = 8  # 64-posting chunks a wave has in flight (kTfK)
TILE = 4096

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(PL.LIB_PATH)
        L.smep_tfsort_last_error.restype, L.smep_tfsort_last_error.argtypes = C.c_char_p, []
        L.smep_tfsort_max_tf.restype, L.smep_tfsort_max_tf.argtypes = _int, []
        L.smep_tf_sort_segments.restype = _int
        L.smep_tf_sort_segments.argtypes = [_vp, _i64, _vp, _vp, _int, _vp, _vp, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def tf_sort_segments(off, docno, tf, max_tf):
    off, docno, tf = PL._c(off, np.int64), PL._c(docno, np.int32), PL._c(tf, np.int32)
    P = int(off[-1])
    assert len(docno) == P and len(tf) == P
    od, ot = np.empty(P, np.int32), np.empty(P, np.int32)
    guard = C.c_int(0)
    rc = lib().smep_tf_sort_segments(PL._p(off), len(off) - 1, PL._p(docno), PL._p(tf), max_tf, PL._p(od), PL._p(ot),
                                     C.byref(guard))
    if rc != 0:
        msg = lib().smep_tfsort_last_error().decode()
        if rc == -2:  # SME_EHIP: the device context may be lost, so nothing more is started on it
            pytest.exit("HIP error in the primitive harness: " + msg, returncode=3)
        raise PL.PrimsError(rc, msg)
    if guard.value:
        raise PL.GuardError("changed: " + ", ".join(n for i, n in enumerate(GUARDS) if guard.value >> i & 1))
    return od, ot


def reference(off, docno, tf):
    od, ot = np.empty_like(docno), np.empty_like(tf)
    for s in range(len(off) - 1):
        b, e = int(off[s]), int(off[s + 1])
        p = np.argsort(-tf[b:e], kind="stable")
        od[b:e], ot[b:e] = docno[b:e][p], tf[b:e][p]
    return od, ot


# every class boundary, the tile boundaries, a five-tile segment with a 63-posting
# tail, and K * 64 - 1, K * 64, K * 64 + 1 where each class batches: the wave class
# itself, a medium segment's four waves (4 * K * 64), a large segment's last tile,
# and that tile's 1024-posting count batches
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193,
           8192 + TILE - 1, 8192 + TILE, 8192 + TILE + 1, 5 * TILE + 63,
           K * 64 - 1, K * 64, K * 64 + 1,
           4 * K * 64 - 1, 4 * K * 64, 4 * K * 64 + 1,
           3 * TILE + K * 64 - 1, 3 * TILE + K * 64, 3 * TILE + K * 64 + 1,
           3 * TILE + 1023, 3 * TILE + 1024, 3 * TILE + 1025]


def klass(n):
    return 0 if n <= 8 else 1 if n <= 64 else 2 if n <= 512 else 3 if n <= 8192 else 4


def interleave(lengths):
    """neighbours of different classes, an empty segment after every third"""
    by = [[n for n in lengths if n and klass(n) == c] for c in (4, 0, 3, 1, 2)]
    out = [0]
    while any(by):
        for b in by:
            if b:
                if out[-1] and klass(out[-1]) == klass(b[0]):
                    out.append(0)
                out.append(b.pop(0))
                if len(out) % 4 == 0:
                    out.append(0)
    out.append(0)
    return out


PATTERNS = ("ones", "max", "alternate", "distinct64", "ascending", "descending", "zipf")


def tf_pattern(rng, name, n, m):
    i = np.arange(n, dtype=np.int64)
    if name == "ones":
        t = np.ones(n, np.int64)
    elif name == "max":
        t = np.full(n, m, np.int64)
    elif name == "alternate":
        t = np.where(i % 2 == 0, 1, m)
    elif name == "distinct64":  # i * 37 mod 64 is a permutation of every 64 consecutive i
        t = 1 + (i * 37 % 64) % m
    elif name == "ascending":
        t = 1 + i * m // max(n, 1)
    elif name == "descending":
        t = m - i * m // max(n, 1)
    else:
        t = np.minimum(rng.zipf(2.0, n), m)
    assert n == 0 or (t.min() >= 1 and t.max() <= m)
    return t.astype(np.int32)


def docnos(j, n):
    """ascending within the segment: from INT32_MIN, up to INT32_MAX (the tail past
    2^31 - 2^16), or across zero"""
    i = np.arange(n, dtype=np.int64)
    base = (-(1 << 31), (1 << 31) - n, -(n // 2))[j % 3]
    return (base + i).astype(np.int32)


def make_csr(rng, lengths, pattern, m):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    tf = np.concatenate([tf_pattern(rng, pattern, n, m) for n in lengths] + [np.empty(0, np.int32)])
    dn = np.concatenate([docnos(j, n) for j, n in enumerate(lengths)] + [np.empty(0, np.int32)])
    return off, dn, tf


def check(off, dn, tf, m, tag):
    assert int(off[-1]) <= 1_100_000
    dn0, tf0 = dn.copy(), tf.copy()
    od, ot = tf_sort_segments(off, dn, tf, m)
    assert np.array_equal(dn, dn0) and np.array_equal(tf, tf0)
    rd, rt = reference(off, dn, tf)
    bad = np.flatnonzero((od != rd) | (ot != rt))
    if len(bad):
        s = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise AssertionError("%s: %d postings differ, first at %d: segment %d of length %d, offset %d" % (
            tag, len(bad), bad[0], s, off[s + 1] - off[s], bad[0] - off[s]))


MAX_TFS = [1, 2, 63, 64, 1023]


def test_limits():
    assert lib().smep_tfsort_max_tf() == 1023


@pytest.mark.parametrize("m", MAX_TFS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_lengths_and_patterns(pattern, m):
    rng = np.random.default_rng(7100 + m)
    lengths = interleave(LENGTHS)
    assert sorted(n for n in lengths if n) == sorted(n for n in LENGTHS if n)
    for a, b in zip(lengths, lengths[1:]):
        assert not (a and b) or klass(a) != klass(b)
    off, dn, tf = make_csr(rng, lengths, pattern, m)
    assert {int(off[s]) % 4 for s in range(len(lengths)) if lengths[s] > 8192} == {0, 1, 2, 3}
    check(off, dn, tf, m, (pattern, m))


@pytest.mark.parametrize("m", MAX_TFS)
def test_no_large_segment(m):
    rng = np.random.default_rng(7200 + m)
    lengths = interleave([n for n in LENGTHS if n <= 8192])
    for pattern in ("zipf", "distinct64"):
        check(*make_csr(rng, lengths, pattern, m), m, ("no large", pattern, m))


@pytest.mark.parametrize("m", MAX_TFS)
def test_only_large_segments(m):
    rng = np.random.default_rng(7300 + m)
    lengths = [n for n in LENGTHS if n > 8192]
    for pattern in ("zipf", "distinct64"):
        check(*make_csr(rng, lengths, pattern, m), m, ("only large", pattern, m))


@pytest.mark.parametrize("m", [2, 63, 1023])
def test_many_large_segments(m):
    """a hundred large segments of three tiles, a tiny one between every two: the
    counters' scan covers 300 tiles x (m + 1) values, up to 75 of its own 4096-value
    tiles, and every segment's positions are taken relative to its own first value"""
    rng = np.random.default_rng(7400 + m)
    lengths = []
    for j in range(100):
        lengths += [8193 + 37 * j, j % 9]
    check(*make_csr(rng, lengths, "zipf", m), m, ("many large", m))


def test_empty():
    """V = 0; and P = 0 over empty segments"""
    e = np.empty(0, np.int32)
    od, ot = tf_sort_segments(np.zeros(1, np.int64), e, e, 5)
    assert len(od) == 0 and len(ot) == 0
    od, ot = tf_sort_segments(np.zeros(6, np.int64), e, e, 5)
    assert len(od) == 0 and len(ot) == 0


def test_bad_max_tf_is_refused():
    off, dn, tf = np.array([0, 3], np.int64), np.arange(3, dtype=np.int32), np.ones(3, np.int32)
    for m in (0, 1024):
        with pytest.raises(PL.PrimsError):
            tf_sort_segments(off, dn, tf, m)
