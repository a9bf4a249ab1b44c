"""term_sort's packed gather mode (csrc/sme_sort.hip: rec_val / tf_shift) against
numpy's stable sort, bit-exact.  The regions hold one word per pair,
term | tf << tf_shift, and rec_val[i] is record i's base value: the first pass
reads the words alone, keys the pair by the low tf_shift bits and gives it the
value rec_val[i] + tf.  Through libsme_prims.so (tests/native/prims_packed.hip),
with the guard and fill discipline of the other primitive tests; the value
buffer v0 must stay untouched unless the sort has three passes or more."""
import ctypes as C

import numpy as np
import pytest

import prims_lib as PL
from test_gpu_prims import GATHER_CASES, TILE, _npass, gather_counts, stable_perm

pytestmark = pytest.mark.gpu

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_ip = C.POINTER(C.c_int)
GUARDS = ("k0", "k1", "v0", "v1", "docno", "tf", "w", "scratch", "v0 written by fewer than three passes")

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(PL.LIB_PATH)
        L.smep_packed_last_error.restype, L.smep_packed_last_error.argtypes = C.c_char_p, []
        L.smep_term_sort_packed.restype = _int
        L.smep_term_sort_packed.argtypes = [_vp, _i64, _i64, _vp, _vp, _vp, _int, _i64, _int, _i64, C.c_uint32, _vp,
                                            _i64, C.c_double, _int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _ip,
                                            _ip]
        _lib = L
    return _lib


def term_sort_packed(words, reg, xoff, rec_val, tf_shift, P, bits, dmin, F, lut=None, idf=0.0, maxbits=11, xw=None,
                     Pout=0):
    words, rec_val = PL._c(words, np.uint32), PL._c(rec_val, np.uint32)
    reg, xoff, lut, xw = PL._c(reg, np.int64), PL._c(xoff, np.int64), PL._c(lut, np.float64), PL._c(xw, np.uint32)
    nout = max(P, Pout)
    ok, od, ot = np.empty(nout, np.uint32), np.empty(nout, np.int32), np.empty(nout, np.int32)
    ow = None if lut is None else np.empty(nout, np.float64)
    which, guard = C.c_int(-2), C.c_int(0)
    p = PL._p
    rc = lib().smep_term_sort_packed(p(words), len(words), len(reg), p(reg), p(xoff), p(rec_val), tf_shift, P, bits,
                                     dmin, F, p(lut), 0 if lut is None else len(lut), idf, maxbits, p(xw),
                                     0 if xw is None else len(xw), Pout, nout, p(ok), p(od), p(ot), p(ow),
                                     C.byref(which), C.byref(guard))
    if rc != 0:
        msg = lib().smep_packed_last_error().decode()
        if rc == -2:  # SME_EHIP: the device context may be lost, so nothing more is started on it
            pytest.exit("HIP error in the primitive harness: " + msg, returncode=3)
        raise PL.PrimsError(rc, msg)
    if guard.value:
        raise PL.GuardError("changed: " + ", ".join(n for i, n in enumerate(GUARDS) if guard.value >> i & 1))
    return dict(keys=ok, docno=od, tf=ot, w=ow, which=which.value)


def packed_layout(rng, cnt, words):
    """regions with gaps between them, not in ascending address order; junk in the
    gaps and around the regions"""
    cnt = np.asarray(cnt, np.int64)
    xoff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    order = rng.permutation(len(cnt))
    gaps = rng.integers(0, 8, len(cnt))
    reg = np.zeros(len(cnt), np.int64)
    pos = 3
    for j in order:
        reg[j] = pos
        pos += int(cnt[j]) + int(gaps[j])
    src = rng.integers(0, 1 << 32, pos + 5, dtype=np.uint32)
    rec = np.repeat(np.arange(len(cnt)), cnt)
    src[reg[rec] + np.arange(len(words)) - xoff[rec]] = words
    return src, reg, xoff, rec


def check_packed(rng, cnt, bits, maxbits, F, dmin, with_w=True, W=0):
    """cnt: pairs per record.  The tf field is every bit above the key
    (tf_shift + tf width == 32) and holds values up to its top; F is a power of
    two no smaller than the field, or any F > the largest tf drawn."""
    P = int(np.sum(cnt))
    tfw = 32 - bits
    nterm = W if W else 1 << bits
    keys = rng.integers(0, nterm, P, dtype=np.uint32)
    if P > 2:
        keys[: P // 3] = np.minimum(rng.zipf(1.3, P // 3), nterm).astype(np.uint32) - np.uint32(1)
    tf_hi = min(1 << tfw, F)
    tfs = rng.integers(0, tf_hi, P, dtype=np.uint32)
    tfs[rng.integers(0, P, max(1, P // 50))] = tf_hi - 1  # the top of the field
    words = keys | (tfs.astype(np.uint64) << np.uint64(bits)).astype(np.uint32)
    src, reg, xoff, rec = packed_layout(rng, cnt, words)
    rec_val = (rng.integers(0, ((1 << 32) - tf_hi) // F + 1, len(cnt)) * F).astype(np.uint32)  # (docno - dmin) * F
    vals = (rec_val[rec].astype(np.int64) + tfs).astype(np.int64)
    assert P == 0 or int(vals.max()) < 1 << 32
    lut = 1.0 + rng.random(F) if with_w else None
    xw, Pout = None, 0
    if W:
        ins = rng.integers(0, 4, W) * (rng.random(W) < 0.3)
        xw = np.empty((W, 2), np.uint32)
        xw[:, 0] = np.cumsum(ins)
        xw[:, 1] = rng.integers(0, 0xFFFFFFFF, W, dtype=np.uint32)
        Pout = P + int(xw[-1, 0]) + 3
    r = term_sort_packed(src, reg, xoff, rec_val, bits, P, bits, dmin, F, lut=lut, idf=3.25, maxbits=maxbits, xw=xw,
                         Pout=Pout)
    tag = (P, bits, maxbits, W)
    assert r["which"] == _npass(bits, 4, maxbits) % 2, tag
    perm = stable_perm(keys, bits)
    sk, sv = keys[perm], vals[perm]
    docno, tf = (sv // F + dmin).astype(np.int32), (sv % F).astype(np.int32)
    n = max(P, Pout)
    if xw is None:
        slot = np.arange(P)
        assert np.array_equal(r["keys"], sk), tag  # the key alone: no tf bits above it
    else:
        slot = np.arange(P) + xw[sk, 0].astype(np.int64)
        ek = np.full(Pout, 0xFFFFFFFF, np.uint32)
        ek[slot] = xw[sk, 1]
        assert np.array_equal(r["keys"], ek), tag
    ed, et = np.full(n, PL.FILL_I32, np.int32), np.full(n, PL.FILL_I32, np.int32)
    ed[slot], et[slot] = docno, tf
    assert np.array_equal(r["docno"], ed), tag
    assert np.array_equal(r["tf"], et), tag
    if lut is not None:
        ew = np.full(n, PL.FILL_U64, np.uint64)
        ew[slot] = (lut[tf] * np.float64(3.25)).view(np.uint64)
        assert np.array_equal(r["w"].view(np.uint64), ew), tag


def small_records(rng, P):
    """records of 1 to 20 pairs summing to P: more than 48 of them in a wave's
    1024 items, so the walk leaves the LDS table for the global one"""
    c = []
    while sum(c) < P:
        c.append(int(rng.integers(1, 21)))
    c[-1] -= sum(c) - P
    return c


# one, two and four passes.  The first and the last fill the tf field to its top
# (F = 2^(32 - bits)); the second has an F that is no power of two and a large dmin
PASSES = ((11, 11, 1 << 21, 0), (13, 11, 65537, 2_000_000_000), (22, 6, 1 << 10, 17))
SIZES = [1, 2, 8191, 8192, 8193, 9 * TILE + 1]


@pytest.mark.parametrize("P", SIZES)
def test_packed_sizes(P):
    rng = np.random.default_rng(9100 + P)
    for i, (bits, maxbits, F, dmin) in enumerate(PASSES):
        check_packed(rng, small_records(rng, P), bits, maxbits, F, dmin, with_w=(P + i) % 2 == 0)
        check_packed(rng, [P], bits, maxbits, F, dmin)  # one record over every tile


@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_packed_record_shapes(name):
    """runs of empty records, records of exactly a wave's 1024 items, one record
    over several tiles, thousands of small records"""
    rng = np.random.default_rng(9200)
    cnt = gather_counts(rng, name)
    for bits, maxbits, F, dmin in PASSES:
        check_packed(rng, cnt, bits, maxbits, F, dmin)


@pytest.mark.parametrize("maxbits", [11, 6, 4])
def test_packed_docid_slots(maxbits):
    """K6b (xw, Pout) over packed words: one, two / three and three / four passes"""
    rng = np.random.default_rng(9300 + maxbits)
    for P, W in ((1, 1), (1025, 37), (TILE + 1, 5000), (9 * TILE + 1, 1 << 13)):
        bits = max(1, int(W - 1).bit_length())
        cnt = small_records(rng, P) if P > 1025 else [0, 0, P, 0]
        check_packed(rng, cnt, bits, maxbits, 65537, 5, W=W)


def test_packed_empty():
    """P = 0 returns k0 and touches nothing"""
    words = np.arange(100, dtype=np.uint32) * 7
    r = term_sort_packed(words, np.zeros(3, np.int64), np.zeros(4, np.int64), np.zeros(3, np.uint32), 11, 0, 11, 0,
                         1000, lut=np.ones(1000), idf=1.0, Pout=100)
    assert r["which"] == 0
    assert np.array_equal(r["keys"], words)
    assert np.all(r["docno"] == PL.FILL_I32) and np.all(r["tf"] == PL.FILL_I32)
    assert np.all(r["w"].view(np.uint64) == PL.FILL_U64)
